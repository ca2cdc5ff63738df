"""The mip-chain generator (include/sah_mip_chain.h) without a GPU: the export and the header, the level counts of the façade's formulas,
every refusal on a context without a device, and the numpy restatement (tests/mip_chain_ref.py) against the committed fixtures, the
second restatement of tools/gen_golden_mip_chain.py and properties one can state without running either."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib
from tests import mip_chain_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mip_chain as gen  # noqa: E402

D32, R32, R16, RGBA16, B10 = ref.FORMAT_D32, ref.FORMAT_R32, ref.FORMAT_R16, ref.FORMAT_RGBA16, ref.FORMAT_B10G11R11
f16, f32 = np.float16, np.float32


# ---- export, header, level counts -------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.MIP_CHAIN_EXPORTS)
    header = open(os.path.join(ROOT, "include", "sah_mip_chain.h")).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.MIP_CHAIN_EXPORTS) == ["sah_mip_chain_generate"]
    assert not set(lib.MIP_CHAIN_EXPORTS) & set(lib.EXPORTS)
    assert "mip_chain" not in open(os.path.join(ROOT, "include", "sah_hip.h")).read()  # sah_hip.h and its ABI version stay as they are
    assert "parity unpinned" in header.lower() and header.count("ABI-defined") >= 6
    # culling and the draw lists are out of scope: no such entry anywhere in the library
    assert not [s for s in ("sah_hi_z_cull", "sah_depth_culling", "sah_visibility_list_to_draw_commands", "sah_init_count_buffer") if hasattr(L, s)]


@pytest.mark.parametrize("language", ["c", "c++"])
def test_header_compiles(tmp_path, language):
    src = tmp_path / ("use.c" if language == "c" else "use.cpp")
    check = "_Static_assert" if language == "c" else "static_assert"
    src.write_text('#include "sah_mip_chain.h"\n'
                   f'{check}(SAH_MIP_CHAIN_MAX_LEVELS == 12 && SAH_MIP_CHAIN_MAX_SOURCE == 4096, "SPD limits");\n'
                   "int use(sah_ctx* c, const sah_plane* s, const sah_plane* d) { return sah_mip_chain_generate(c, s, d, 7); }\n")
    clang = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else "cc"
    subprocess.check_call([clang, "-x", language, "-std=c11" if language == "c" else "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)], timeout=120)
    assert lib.MIP_CHAIN_MAX_LEVELS == 12 and lib.MIP_CHAIN_MAX_SOURCE == 4096


@pytest.mark.parametrize("resolution,hi_z_levels,spd_levels", [((1280, 720), 9, 10), ((1920, 1080), 10, 10), ((3840, 2160), 11, 11)])
def test_level_counts_of_the_facade_formulas(resolution, hi_z_levels, spd_levels):
    extent, levels = ref.hi_z_extent_and_levels(resolution)
    assert extent == (resolution[0] // 2, resolution[1] // 2) and levels == hi_z_levels
    assert ref.spd_mips(*resolution) == spd_levels
    # the façade's own text computes the same two numbers (include/sah_host.hpp: DepthCullingPhase::set_render_resolution)
    text = open(os.path.join(ROOT, "include", "sah_host.hpp")).read()
    assert "std::round(std::log2((float)major_dimension))" in text and "resolution[0] / 2" in text


def test_the_lane_map_and_the_workgroup_geometry():
    x, y = ref.armp_red8x8(np.arange(64))
    assert sorted(zip(x.tolist(), y.tolist())) == [(i, j) for i in range(8) for j in range(8)]  # a bijection onto 8 x 8
    a = np.arange(64)
    assert ((x ^ 1) == ref.armp_red8x8(a ^ 1)[0]).all() and (y == ref.armp_red8x8(a ^ 1)[1]).all()   # lane ^ 1: the horizontal neighbour
    assert (x == ref.armp_red8x8(a ^ 2)[0]).all() and ((y ^ 1) == ref.armp_red8x8(a ^ 2)[1]).all()   # lane ^ 2: the vertical one
    assert [ref.spd_mips(w, h) for w, h in ((1, 1), (2, 2), (3, 1), (64, 64), (127, 5), (128, 128), (4096, 1), (4095, 4095))] == [0, 1, 1, 6, 6, 7, 12, 11]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
OK, INVALID, FORMAT = "well-formed", _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT


def _plane(ptr, fmt, w, h, pitch=None):
    return _abi.Plane(ptr, w, h, w * _abi.FORMAT_BPP.get(fmt, 4) if pitch is None else pitch, fmt)


def _chain_planes(base, fmt, extent0, n):
    return [_plane(base + (i << 20), fmt, w, h) for i, (w, h) in enumerate(ref.level_extents(extent0, n))]


def _cases(base):
    src = _plane(base, D32, 128, 128)
    L = lambda n=7, fmt=R32, e=(64, 64): _chain_planes(base + (1 << 26), fmt, e, n)  # noqa: E731

    def changed(i, n=7, **kw):
        out = L(n)
        for k, v in kw.items():
            setattr(out[i], k, v)
        return out
    yield "depth", src, L(), OK
    yield "R32 source", _plane(base, R32, 128, 128), L(), OK
    yield "more levels than SPD makes", src, L(12, e=(2048, 2048)), OK
    yield "level 0 of another extent", src, L(e=(100, 40)), OK
    yield "six levels of seven made", _plane(base, D32, 160, 96), L(6, e=(80, 48)), OK
    yield "one level, one made", _plane(base, D32, 2, 2), L(1, e=(1, 1)), OK
    yield "two levels of six made, one workgroup", _plane(base, D32, 64, 64), L(2, e=(32, 32)), OK
    for fmt in (R16, RGBA16, B10):
        yield f"format {fmt}", _plane(base, fmt, 128, 128), L(fmt=fmt), OK
        yield f"format {fmt} into R32", _plane(base, fmt, 128, 128), L(), FORMAT
        yield f"depth into format {fmt}", src, L(fmt=fmt), FORMAT
    yield "D32 levels", src, L(fmt=D32), FORMAT
    yield "R8G8B8A8 source", _plane(base, _abi.FORMAT_R8G8B8A8_UNORM, 128, 128), L(), FORMAT
    yield "mixed level formats", src, changed(3, format=B10), FORMAT
    yield "null source", None, L(), INVALID
    yield "null source pointer", _plane(None, D32, 128, 128), L(), INVALID
    yield "null level array", src, None, INVALID
    yield "null level pointer", src, changed(2, ptr=None), INVALID
    yield "zero source width", _plane(base, D32, 0, 128), L(), INVALID
    yield "zero source height", _plane(base, D32, 128, 0), L(), INVALID
    yield "zero level extent", src, changed(0, width=0), INVALID
    yield "no levels", src, [], INVALID
    yield "thirteen levels", src, _chain_planes(base + (1 << 26), R32, (4096, 4096), 13), INVALID
    yield "level 2 one texel wider", src, changed(2, width=17, row_pitch_bytes=68), INVALID
    yield "level 6 is 2 x 1", src, changed(6, width=2, row_pitch_bytes=8), INVALID
    yield "level 1 one row short", src, changed(1, height=31), INVALID
    yield "short source pitch", _plane(base, D32, 128, 128, 508), L(), INVALID
    yield "short level pitch", src, changed(1, row_pitch_bytes=124), INVALID
    yield "misaligned source", _plane(base + 2, D32, 128, 128), L(), INVALID
    yield "misaligned level", src, changed(4, ptr=base + (1 << 26) + (4 << 20) + 1), INVALID
    yield "RGBA16F level aligned to 4 only", _plane(base, RGBA16, 128, 128), [_plane(p.ptr + 4, RGBA16, p.width, p.height) for p in L(fmt=RGBA16)], INVALID
    yield "source pitch not a multiple of 4", _plane(base, D32, 128, 128, 514), L(), INVALID
    yield "source wider than 4096", _plane(base, D32, 4097, 8), L(), INVALID
    yield "source taller than 4096", _plane(base, D32, 8, 4097), L(), INVALID
    yield "one level, several made", src, L(1), INVALID
    yield "level 5 missing, seven made", src, L(5), INVALID
    yield "two levels of six made, four workgroups", _plane(base, D32, 100, 100), L(2, e=(50, 50)), INVALID


def test_every_refusal_of_the_header_on_a_context_without_a_device():
    """A malformed call answers its status; a well-formed one gets as far as selecting the device, which a detached context does not have
    (SAH_ERR_HIP) — so nothing is launched and the made-up addresses are never used."""
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        pytest.skip("a HIP device is present (made-up addresses must not reach a GPU); tests/test_mip_chain_gpu.py checks the refusals there")
    n = 0
    try:
        for name, src, levels, want in _cases(0x10000000):
            arr = None if levels is None else (_abi.Plane * max(len(levels), 1))(*levels)
            got = L.sah_mip_chain_generate(h, None if src is None else C.byref(src), arr, 7 if levels is None else len(levels))
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"{name}: status {got}"
            n += 1
        _, src, levels, _ = next(_cases(0x10000000))
        assert L.sah_mip_chain_generate(None, C.byref(src), (_abi.Plane * 7)(*levels), 7) == INVALID
    finally:
        L.sah_destroy(h)
    assert n > 40


# ---- restatements and fixtures ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures():
    return {tag: np.load(gen.fixture_path(tag)) for tag in gen.CASES}


def _fixture_levels(fx, name):
    return [fx[f"{name}_level{i}"] for i in range(int(fx["num_levels"]))]


@pytest.mark.parametrize("tag", list(gen.CASES))
def test_ref_reproduces_the_fixture_and_the_generator_its_inputs(fixtures, tag):
    fx = fixtures[tag]
    size, extent0, n = gen.CASES[tag]
    assert tuple(fx["extent0"]) == extent0 and int(fx["num_levels"]) == n and os.path.getsize(gen.fixture_path(tag)) < 1024 * 1024
    srcs = gen.inputs(size, int(fx["seed"]))
    for fmt, name in gen.NAMES.items():
        assert srcs[fmt].tobytes() == fx[f"{name}_src"].tobytes(), name
        got = ref.generate(fx[f"{name}_src"], fmt, extent0, n)
        for i, want in enumerate(_fixture_levels(fx, name)):
            assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), (name, i)


def test_the_geometric_restatement_agrees_and_neither_imports_the_other(fixtures):
    fx = fixtures["192x136"]
    for fmt, name in gen.NAMES.items():
        got = gen.chain(fx[f"{name}_src"], fmt, (96, 68), 7)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, _fixture_levels(fx, name))), name
    # shapes the fixtures do not hold: an odd source, levels 7 and 8, a level 0 that is not half the source
    g = np.random.default_rng(2)
    for size, extent0, n in (((131, 67), (65, 33), 7), ((320, 200), (160, 100), 8), ((128, 128), (100, 40), 7), ((64, 64), (32, 32), 3)):
        src = g.random((size[1], size[0]), dtype=f32)
        a, b = gen.chain(src, D32, extent0, n), ref.generate(src, D32, extent0, n)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b)), size
    ref_text = open(os.path.join(ROOT, "tests", "mip_chain_ref.py")).read()
    chain_text = open(os.path.join(ROOT, "tools", "gen_golden_mip_chain.py")).read()
    assert "gen_golden" not in ref_text.split('"""', 2)[2]
    body = chain_text[chain_text.index("# ---- the geometric restatement"):chain_text.index("def generate(")]
    assert "mip_chain_ref" not in body.replace("tests/mip_chain_ref.py", "")


def test_what_the_fixture_inputs_hold(fixtures):
    for tag, fx in fixtures.items():
        d = fx["d32_src"]
        bits = d.view(np.uint32)
        assert bits[gen.PLANTED["inf"][1], gen.PLANTED["inf"][0]] == 0x7f800000 and bits[gen.PLANTED["nan"][1], gen.PLANTED["nan"][0]] == 0x7fc00000
        assert np.isinf(d).sum() == 1 and np.isnan(d).sum() == 1
        finite = d[np.isfinite(d)]
        assert (finite == 0).sum() > 100 and ((finite > 0) & (finite < 6.1e-5)).sum() > 100 and finite.min() >= 0 and finite.max() <= 1   # sky, fp16 subnormals, reversed-Z
        assert ((bits & 0x1fff) == 0x1000).sum() > 100                                                 # halfway between two halves
        for name in ("r16", "rgba16"):
            h = fx[f"{name}_src"]
            assert set(((h >> 10) & 31).ravel().tolist()) == set(range(31)) and (h & 0x8000).any()    # every exponent, both signs, no inf / NaN
        assert set(((fx["b10g11r11_src"] >> 6) & 31).ravel().tolist()) == set(range(31))
        # the levels hold what the inputs were chosen for: subnormal halves, +inf, and no NaN past level 1 of the depth chain
        l0 = fx["d32_level0"].view(f32)
        assert ((l0 > 0) & (l0 < 6.1e-5)).any() and np.isinf(l0).any() and np.isnan(l0).any() and not np.isnan(fx["d32_level2"].view(f32)).any()


# ---- properties -----------------------------------------------------------------------------------------------------------------------------
def _block_min(a, k):
    h, w = a.shape
    return a[:h - h % k, :w - w % k].reshape(h // k, k, w // k, k).min(axis=(1, 3))


def test_depth_levels_are_block_minima_of_level_0():
    g = np.random.default_rng(4)
    src = (0.05 / (0.3 + 40 * g.random((128, 128)) ** 3)).astype(f32)
    src[g.random((128, 128)) < 0.2] = 0
    levels = [lv.view(f32) for lv in ref.generate(src, D32, (64, 64), 7)]
    assert [lv.shape for lv in levels] == [(64 >> i, 64 >> i) for i in range(7)]
    for k in range(1, 7):
        assert np.array_equal(levels[k], _block_min(levels[0], 1 << k)), k
    # level 0 is a SAMPLE, never a min: a checkerboard of 0 and 1 gives 0.5 everywhere
    board = ((np.add.outer(np.arange(128), np.arange(128)) & 1)).astype(f32)
    assert (ref.generate(board, D32, (64, 64), 7)[0].view(f32) == 0.5).all()


@pytest.mark.parametrize("fmt,value", [(R16, 0.3), (RGBA16, 1234.0), (B10, 7.25), (R16, 3e-6)])
def test_a_constant_source_yields_the_constant_at_every_level(fmt, value):
    v = f16(value)
    shape = (128, 128, 4) if fmt == RGBA16 else (128, 128)
    if fmt == B10:
        b = int(v.view(np.uint16))
        src = np.full(shape, (b >> 4) | ((b >> 4) << 11) | ((b >> 5) << 22), np.uint32)
    else:
        src = np.full(shape, v.view(np.uint16), np.uint16)
    levels = ref.generate(src, fmt, (64, 64), 7)
    for i, lv in enumerate(levels):
        assert lv.shape[:2] == (64 >> i, 64 >> i)
        got = ref.decode(lv, fmt)
        assert (got == v).all(), (i, got.ravel()[:4])
    # where level 6 reads outside level 5 (2 x 1 at 160 x 96 into 80 x 48) the zeros read there are part of the mean
    if fmt == R16:
        src = np.full((96, 160), v.view(np.uint16), np.uint16)
        levels = ref.generate(src, fmt, (80, 48), 7)
        assert all((ref.decode(lv, fmt) == v).all() for lv in levels[:6])
        assert ref.decode(levels[6], fmt).ravel()[0] == f16(f16(v + v) * f16(0.25))


def test_the_stray_store_of_160x96():
    fx = np.load(gen.fixture_path("160x96"))
    src = fx["d32_src"]
    stray = ref.generate(src, D32, (80, 48), 6)
    clean = ref.generate(src, D32, (80, 48), 7)
    assert ref.spd_mips(160, 96) == 7
    assert stray[1][0, 0] == clean[6][0, 0]  # the restated level-6 value
    rest = np.ones(stray[1].shape, bool)
    rest[0, 0] = False
    assert np.array_equal(stray[1][rest], clean[1][rest])
    for i in (0, 2, 3, 4, 5):
        assert np.array_equal(stray[i], clean[i])
    # level 6 = min over stored level 5 (2 x 1) and the zeros outside it, below before right
    assert clean[6][0, 0] == 0 and clean[1][0, 0] != 0


def test_fma32_rounds_once():
    from fractions import Fraction
    g = np.random.default_rng(8)
    a = g.standard_normal(4000).astype(f32) * f32(1e-3)
    b = g.standard_normal(4000).astype(f32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + g.integers(-3, 4, 4000) * 2.0 ** -24)).astype(f32)  # cancellation: the low bits decide
    got = ref.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = f32(float(exact))  # (float(Fraction) is correctly rounded to fp64; 53 bits suffice here only as a starting point)
        cands = [np.nextafter(lo, f32(-np.inf)), lo, np.nextafter(lo, f32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(f32(v).view(np.uint32)) & 1))
        assert got[i] == best, i
    assert ref.fma32(f32(1 + 2 ** -23), f32(1 + 2 ** -23), -f32(1 + 2 ** -22)) == f32(2 ** -46)  # a rounded product would leave 0
