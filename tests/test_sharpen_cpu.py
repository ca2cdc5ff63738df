"""Contrast-adaptive sharpening (include/sah_sharpen.h) without a GPU: the export and the header, the 12-byte structure, every refusal the
header lists on a context without a device, an argument fuzz in a child process, and the numpy restatement (tests/sharpen_ref.py) — its
committed fixture and the properties that make it a sharpening filter."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib
from tests import sharpen_ref as ref
from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_sharpen as gen  # noqa: E402

f32 = np.float32
RGBA16F = _abi.FORMAT_R16G16B16A16_SFLOAT
HEADER = os.path.join(ROOT, "include", "sah_sharpen.h")
PARAM_FIELDS = ["sharpness", "pre_scale", "flags"]


# ---- exports, header, structure -----------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.SHARPEN_EXPORTS)
    header = open(HEADER).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.SHARPEN_EXPORTS) == ["sah_sharpen"]
    assert not set(lib.SHARPEN_EXPORTS) & set(lib.EXPORTS)
    hip_h = open(os.path.join(ROOT, "include", "sah_hip.h")).read()
    assert "sah_sharpen" not in hip_h and re.search(r"#define\s+SAH_ABI_VERSION\s+6\b", hip_h)  # sah_hip.h's declarations and ABI version stay
    assert "ABI-defined" in header and "NOT part of it" in " ".join(header.split())
    assert re.search(r"#define\s+SAH_SHARPEN_DENOISE\s+1u\b", header) and _abi.SHARPEN_DENOISE == ref.DENOISE == 1


@pytest.mark.parametrize("language", ["c", "c++"])
def test_header_compiles_and_the_structure_is_12_bytes(tmp_path, language):
    src = tmp_path / ("use.c" if language == "c" else "use.cpp")
    check = "_Static_assert" if language == "c" else "static_assert"
    offsets = "".join(f'{check}(offsetof(sah_sharpen_params, {n}) == {4 * i}, "{n}");\n' for i, n in enumerate(PARAM_FIELDS))
    src.write_text('#include <stddef.h>\n#include "sah_sharpen.h"\n'
                   f'{check}(sizeof(sah_sharpen_params) == 12, "sah_sharpen_params");\n' + offsets +
                   "int use(sah_ctx* c, const sah_plane* p, const sah_exposure_state* s, const sah_sharpen_params* q) {\n"
                   "    return sah_sharpen(c, p, s, p, q, 0, 0) + (int)SAH_SHARPEN_DENOISE; }\n")
    clang = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else "cc"
    subprocess.check_call([clang, "-x", language, "-std=c11" if language == "c" else "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)], timeout=120)
    assert C.sizeof(_abi.SharpenParams) == 12
    assert [(n, getattr(_abi.SharpenParams, n).offset) for n, _ in _abi.SharpenParams._fields_] == [(n, 4 * i) for i, n in enumerate(PARAM_FIELDS)]
    d = _abi.SharpenParams.default()
    assert {n: getattr(d, n) for n in PARAM_FIELDS} == ref.DEFAULTS
    assert _abi.SharpenParams.default(sharpness=0.25, flags=1).sharpness == 0.25 and _abi.SharpenParams.default(flags=1).flags == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
OK, INVALID, FORMAT = "well-formed", _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
W, H = 24, 16
SIZE = (H - 1) * W * 8 + W * 8


def _plane(base, w=W, h=H, pitch=None, ptr=True, offset=0, fmt=RGBA16F):
    return _abi.Plane((base + offset) if ptr else None, w, h, w * 8 if pitch is None else pitch, fmt)


def _cases(base):
    """(name, (scene, exposure, out, params, row_begin, row_end), expected)"""
    scene_at, out_at, st = base, base + (1 << 16), base + (3 << 16)
    P = _abi.SharpenParams.default

    def call(rows=(0, 0), params="default", **kw):
        a = dict(scene=_plane(scene_at), exposure=st, out=_plane(out_at), params=P() if params == "default" else params)
        a.update(kw)
        return (a["scene"], a["exposure"], a["out"], a["params"]) + tuple(rows)
    yield "whole", call(), OK
    yield "without an exposure", call(exposure=None), OK
    yield "band", call((3, 9)), OK
    yield "empty band", call((5, 5)), OK
    yield "last row", call((H - 1, H)), OK
    yield "padded pitches", call(scene=_plane(scene_at, pitch=W * 8 + 12), out=_plane(out_at, pitch=W * 8 + 4)), OK
    yield "limits of the ranges", call(params=P(sharpness=0.0, pre_scale=1e-38, flags=_abi.SHARPEN_DENOISE)), OK
    yield "a large pre_scale", call(params=P(sharpness=1.0, pre_scale=3e38)), OK
    yield "out ends where the scene begins", call(out=_plane(scene_at - SIZE)), OK
    yield "out begins where the scene ends", call(out=_plane(scene_at + SIZE)), OK
    yield "the exposure ends where out begins", call(exposure=out_at - 16), OK
    yield "the exposure inside the scene", call(exposure=scene_at + 16), OK  # (both are only read)
    for name in ("scene", "out", "params"):
        yield f"{name} NULL", call(**{name: None}), INVALID
    for n, at in (("scene", scene_at), ("out", out_at)):
        yield f"{n}: null pointer", call(**{n: _plane(at, ptr=False)}), INVALID
        yield f"{n}: wrong format", call(**{n: _plane(at, fmt=_abi.FORMAT_R32_SFLOAT)}), FORMAT
        yield f"{n}: short pitch", call(**{n: _plane(at, pitch=W * 8 - 4)}), INVALID
        yield f"{n}: misaligned pointer", call(**{n: _plane(at, offset=2)}), INVALID
        yield f"{n}: pitch not a multiple of 4", call(**{n: _plane(at, pitch=W * 8 + 2)}), INVALID
        yield f"{n}: zero width", call(**{n: _plane(at, w=0)}), INVALID
        yield f"{n}: zero height", call(**{n: _plane(at, h=0)}), INVALID
        yield f"{n}: other width", call(**{n: _plane(at, w=W - 1)}), INVALID
        yield f"{n}: other height", call(**{n: _plane(at, h=H + 1)}), INVALID
    yield "both zero width", call(scene=_plane(scene_at, w=0), out=_plane(out_at, w=0)), INVALID
    yield "2^32 texels", call(scene=_plane(scene_at, w=65536, h=65536, pitch=65536 * 8), out=_plane(base + (1 << 40), w=65536, h=65536, pitch=65536 * 8)), INVALID
    yield "row_begin > row_end", call((9, 3)), INVALID
    yield "row_end > H", call((0, H + 1)), INVALID
    yield "exposure misaligned", call(exposure=st + 2), INVALID
    nan, inf = float("nan"), float("inf")
    for v in (-0.001, 1.001, -1.0, 2.0, inf, -inf, nan):
        yield f"sharpness {v}", call(params=P(sharpness=v)), INVALID
    for v in (0.0, -0.0, -1.0, inf, -inf, nan):
        yield f"pre_scale {v}", call(params=P(pre_scale=v)), INVALID
    for flags in (2, 3, 0x80000000):
        yield f"flags {flags:#x}", call(params=P(flags=flags)), INVALID
    # overlaps: in place is refused, because the pass reads neighbours
    yield "in place", call(out=_plane(scene_at)), INVALID
    yield "out is the scene's memory with another pitch", call(scene=_plane(scene_at, pitch=W * 8 + 8), out=_plane(scene_at)), INVALID
    yield "out ends inside the scene", call(out=_plane(scene_at - SIZE + 4)), INVALID
    yield "out begins inside the scene", call(out=_plane(scene_at + SIZE - 4)), INVALID
    yield "the exposure inside out", call(exposure=out_at + 32), INVALID
    yield "the exposure ends inside out", call(exposure=out_at - 12), INVALID
    yield "the exposure begins inside out", call(exposure=out_at + SIZE - 4), INVALID


def test_every_refusal_of_the_header_on_a_context_without_a_device():
    """A malformed call answers its status; a well-formed one gets as far as selecting the device, which a detached context does not have
    (SAH_ERR_HIP) — so nothing is launched and the made-up addresses are never used."""
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        pytest.skip("a HIP device is present (made-up addresses must not reach a GPU); tests/test_sharpen_gpu.py checks the refusals there")
    ref_of = lambda a: None if a is None else C.byref(a)  # noqa: E731
    n = 0
    try:
        for name, (scene, exposure, out, params, r0, r1), want in _cases(0x10000000):
            got = L.sah_sharpen(h, ref_of(scene), exposure, ref_of(out), ref_of(params), r0, r1)
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"{name}: status {got}"
            n += 1
        scene, exposure, out, params, r0, r1 = next(_cases(0x10000000))[1]
        assert L.sah_sharpen(None, C.byref(scene), exposure, C.byref(out), C.byref(params), 0, 0) == INVALID
    finally:
        L.sah_destroy(h)
    assert n > 60


@pytest.mark.parametrize("seed", [41])
def test_no_argument_combination_crashes_the_entry(seed):
    stdout = support.run_fuzz_child("sharpen_fuzz_child.py", seed, 2000)
    assert "SAH_OK" not in stdout  # (a detached context never launches)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(gen.FIXTURE)


def test_generator_reproduces_the_committed_fixture(fixture):
    got = gen.generate(int(fixture["seed"]))
    assert sorted(got) == sorted(fixture.files)
    for k in fixture.files:
        assert np.asarray(got[k]).dtype == fixture[k].dtype and np.asarray(got[k]).tobytes() == fixture[k].tobytes(), k
    Wf, Hf = gen.WIDTH, gen.HEIGHT
    assert (Wf, Hf) == (69, 21) and Wf % ref.TILE[0] and Hf % ref.TILE[1] and Wf % 2 == 1 and Wf > ref.TILE[0] and Hf > ref.TILE[1]
    assert fixture["scene_plane"].shape == (Hf, gen.PITCH, 4) and (fixture["scene_plane"][:, Wf:] == 0xA5A5).all()
    assert fixture["sharpened"].shape == (len(gen.CASES), Hf, Wf, 4)
    assert os.path.getsize(gen.FIXTURE) < 128 * 1024


def test_the_fixture_takes_every_branch_it_is_there_for(fixture):
    scene = fixture["scene_plane"][:, :gen.WIDTH]
    outs = fixture["sharpened"]
    # DENOISE on and off, a NULL and a device exposure, both values of sharpness and pre_scale; every case changes the picture its own way
    assert {s["flags"] for _, s in gen.CASES} == {0, ref.DENOISE} and {e for e, _ in gen.CASES} == {None, gen.EXPOSURE}
    assert len({o.tobytes() for o in outs}) == len(gen.CASES)
    assert ref.scale_of(0.25, gen.EXPOSURE) == f32(0.25) * f32(gen.EXPOSURE) != f32(0.25)
    # unclean texels of every kind, a clean -0, two of them on the tile seam; they pass through and so do their plus-shaped neighbours
    c = scene.view(np.float16)[..., :3]
    ok = ref.clean(scene)
    assert np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any() and (c < 0).any()
    assert ((scene[..., :3] == 0x8000).any(-1) & ok).any()
    assert 4 <= (~ok).sum() <= 12 and not ok[15, 63] and not ok[16, 64]
    elig = ref.eligible(scene)
    assert not elig[15, 64] and not elig[16, 63] and elig[14, 64] and 5 * (~ok).sum() >= (~elig).sum() > (~ok).sum()
    for o in outs:
        assert (o[~elig] == scene[~elig]).all() and (o[..., 3] == scene[..., 3]).all()
        assert (o[elig][:, :3] != scene[elig][:, :3]).any(-1).mean() > 0.9


# ---- the properties -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, ref.DENOISE])
@pytest.mark.parametrize("maximum", [1e-3, 1.0, 64.0, 4096.0, 65504.0])
def test_every_eligible_pixel_is_finite_and_not_negative_at_any_image_scale(maximum, flags):
    g = np.random.default_rng(int(maximum * 1000) % 9973 + flags)
    img = g.uniform(0, 1, (33, 47, 4)) ** 3 * maximum
    img[g.random((33, 47)) < 0.1, :3] = 0  # a tenth of the texels zero
    img[3, 5, :3] = maximum
    scene = np.minimum(img, 65504.0).astype(np.float16).view(np.uint16)
    for exposure in (None, 2.0 ** 19, 2.0 ** -19):
        out, o, s, ok = ref.sharpen(scene, exposure, dict(flags=flags), details=True)
        assert ok.all() and np.isfinite(o).all() and (o >= 0).all() and (o <= 65504).all()
        assert (s >= 0).all() and (s <= 1).all()
        halfs = out.view(np.float16)[..., :3]
        assert np.isfinite(halfs).all() and (halfs >= 0).all()


def test_sharpness_zero_is_the_identity_up_to_4096():
    """every non-negative half up to 4096 as the largest channel of a texel (in each of the three places), the others random below it;
    the bound is documented, not more: from 8192 on the cancellation in 1 - m loses it"""
    g = np.random.default_rng(2)
    halfs = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16)
    v = halfs[halfs.astype(f32) <= 4096]
    n = len(v)
    img = np.zeros((9, n, 4), np.float16)
    for r in range(9):
        rgb = np.stack([v, (v.astype(f32) * g.random(n)).astype(np.float16), (v.astype(f32) * g.random(n)).astype(np.float16)], -1)
        img[r, :, :3] = np.roll(rgb, r % 3, -1)
        img[r, :, 3] = g.random(n)
    scene = img.view(np.uint16)
    for flags in (0, ref.DENOISE):
        out = ref.sharpen(scene, None, dict(sharpness=0.0, flags=flags))
        assert out.tobytes() == scene.tobytes()
    # beyond the bound it is not promised, and near the top of the half range it does not hold
    top = np.full((3, 3, 4), np.float16(65504.0)).view(np.uint16)
    top[..., 1] = np.float16(30000.0).view(np.uint16)
    assert ref.sharpen(top, None, dict(sharpness=0.0)).tobytes() != top.tobytes()
    # a clean -0 comes out as +0
    zero = np.zeros((3, 3, 4), np.uint16)
    zero[1, 1, :3] = 0x8000
    assert ref.eligible(zero).all() and (ref.sharpen(zero, None, dict(sharpness=0.0)) == 0).all()


def test_a_step_gains_contrast_and_stays_in_range():
    step = np.zeros((5, 8, 4), np.float16)
    step[:, :4, :3], step[:, 4:, :3] = 0.2, 0.6
    out, o, s, ok = ref.sharpen(step.view(np.uint16), None, None, details=True)
    row = out.view(np.float16)[2, :, 0].astype(np.float64)
    assert ok.all() and (s >= 0).all() and (s <= 1).all()
    assert abs(row[3] - 0.143) < 1e-3 and abs(row[4] - 0.714) < 1e-3  # the two texels at the step: 0.2 | 0.6 becomes 0.143 | 0.714
    assert np.allclose(row[:3], 0.2, atol=2e-4) and np.allclose(row[5:], 0.6, atol=5e-4)  # flat ground stays
    # half the sharpness, half the lobe: between the two
    half = ref.sharpen(step.view(np.uint16), None, dict(sharpness=0.5)).view(np.float16)[2, :, 0].astype(np.float64)
    assert row[3] < half[3] < 0.2 and 0.6 < half[4] < row[4]


def test_denoise_scales_the_lobe_down_where_the_centre_is_an_outlier():
    flat = np.full((5, 5, 4), np.float16(0.25))
    flat[1, 2, :3], flat[3, 2, :3] = 0.2, 0.3  # a ring that is not flat, around a centre that sticks out of it
    flat[2, 2, :3] = 0.5
    scene = flat.view(np.uint16)
    off = ref.sharpen(scene).view(np.float16)[2, 2, 0]
    on = ref.sharpen(scene, None, dict(flags=ref.DENOISE)).view(np.float16)[2, 2, 0]
    assert 0.5 < on < off  # both push the outlier further out; DENOISE by less


@pytest.mark.parametrize("at", [(7, 9), (0, 0), (0, 9), (19, 39), (7, 0)])
@pytest.mark.parametrize("bits", [0x7e00, 0x7c00, 0xbc00])  # NaN, +inf, -1
def test_one_unclean_texel_makes_its_plus_pass_through_and_nothing_else(at, bits):
    scene = ref.blocky_inputs(40, 20, 3)
    base = ref.sharpen(scene)
    assert (base[..., :3] != scene[..., :3]).any(-1).all()  # every pixel is sharpened
    dirty = scene.copy()
    dirty[at[0], at[1], 1] = bits
    out = ref.sharpen(dirty)
    y, x = at
    plus = {(y, x)} | {(yy, xx) for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)) if 0 <= yy < 20 and 0 <= xx < 40}
    changed = {tuple(p) for p in np.argwhere((out != base).any(-1)).tolist()}
    assert changed == plus and len(plus) == 5 - (y in (0, 19)) - (x in (0, 39))
    for p in plus:
        assert (out[p] == dirty[p]).all()
    # -0 is clean: nothing passes through
    zero = scene.copy()
    zero[y, x, 1] = 0x8000
    assert ref.eligible(zero).all()


def test_the_exposure_rule():
    k = ref.scale_of
    assert k(1.0) == 1 and k(0.25, None) == f32(0.25) and k(0.25, 0.375) == f32(0.09375)
    for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0, 2.0 ** 23, 2.0 ** -23, 3e38):
        assert k(0.25, bad) == f32(0.25), bad
    assert k(1.0, 2.0 ** 20) == f32(2.0 ** 20) and k(1.0, 2.0 ** -20) == f32(2.0 ** -20)
    assert k(1.0, np.nextafter(f32(2.0 ** 20), f32(np.inf))) == 1 and k(1.0, np.nextafter(f32(2.0 ** -20), f32(0))) == 1
    # the scale moves the compression, not the picture: a scene and its exposure-compensated twin sharpen alike to within the half rounding
    scene = ref.blocky_inputs(21, 9, 8)
    a = ref.sharpen(scene, None, dict(pre_scale=4.0)).view(np.float16)[..., :3].astype(np.float64)
    b = ref.sharpen(scene, 8.0, dict(pre_scale=0.5)).view(np.float16)[..., :3].astype(np.float64)
    assert np.array_equal(a, b)


# ---- the GPU test's main input ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", [(17, 65), (33, 129), (16, 64)])
def test_the_blocky_input_is_sharpened_almost_everywhere(extent):
    """what keeps the GPU comparison from being a comparison of pass-through: at sharpness 1 at least 90 % of the pixels change bits"""
    w, h = extent
    scene = ref.blocky_inputs(w, h, 100 + w)
    halfs = scene.view(np.float16)[..., :3]
    assert halfs.min() > 0.08 and halfs.max() < 1.0
    for flags in (0, ref.DENOISE):
        out = ref.sharpen(scene, None, dict(flags=flags))
        changed = (out[..., :3] != scene[..., :3]).any(-1).mean()
        assert changed >= 0.9, changed
        assert (out[..., 3] == scene[..., 3]).all()


def test_rows_and_bands_of_the_restatement():
    scene = ref.blocky_inputs(19, 11, 4, unclean=3)
    full = ref.sharpen(scene)
    before = np.full(scene.shape, 0x1234, np.uint16)
    a, b = ref.sharpen(scene, rows=(0, 5), out=before), ref.sharpen(scene, rows=(5, 11), out=before)
    assert (a[5:] == 0x1234).all() and (b[:5] == 0x1234).all() and (a[:5] == full[:5]).all() and (b[5:] == full[5:]).all()
    assert (ref.sharpen(scene, rows=(4, 4), out=before) == before).all()
