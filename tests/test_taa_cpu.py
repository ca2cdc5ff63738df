"""Temporal anti-aliasing (include/sah_taa.h) without a GPU: the export and the header, the 24-byte parameter block, every refusal the
header lists, and the numpy restatement (tests/taa_ref.py) — its properties, its committed fixture with every planted case asserted to take
its branch, the sign of the jitter difference against the fp64 reprojection, and convergence on an analytic scene."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib, scene
from tests import mv_reproject
from tests import taa_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_taa as gen  # noqa: E402

f32 = np.float32
RGBA16F, D32, RG16F = _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16G16_SFLOAT


# ---- exports, header, struct ----------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.TAA_EXPORTS)
    header = open(os.path.join(ROOT, "include", "sah_taa.h")).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.TAA_EXPORTS) == ["sah_taa_resolve"]
    assert not set(lib.TAA_EXPORTS) & set(lib.EXPORTS)
    hip_h = open(os.path.join(ROOT, "include", "sah_hip.h")).read()
    assert "taa" not in hip_h.lower() and re.search(r"#define\s+SAH_ABI_VERSION\s+6\b", hip_h)  # sah_hip.h and its ABI version stay as they are
    assert "under row sharding the history must be whole" in " ".join(header.split()) and "ABI-defined" in header


@pytest.mark.parametrize("language", ["c", "c++"])
def test_header_compiles_and_the_parameter_block_is_24_bytes(tmp_path, language):
    src = tmp_path / ("use.c" if language == "c" else "use.cpp")
    check = "_Static_assert" if language == "c" else "static_assert"
    src.write_text('#include "sah_taa.h"\n'
                   f'{check}(sizeof(sah_taa_params) == 24, "sah_taa_params");\n'
                   f'{check}(SAH_TAA_HISTORY_INVALID == 1u && SAH_TAA_HDR_WEIGHTS == 2u, "flags");\n'
                   "int use(sah_ctx* c, const sah_plane* p, const sah_taa_params* s) { return sah_taa_resolve(c, p, p, p, p, p, s, 0, 0); }\n")
    clang = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else "cc"
    subprocess.check_call([clang, "-x", language, "-std=c11" if language == "c" else "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)], timeout=120)
    assert C.sizeof(_abi.TaaParams) == 24 and (_abi.TAA_HISTORY_INVALID, _abi.TAA_HDR_WEIGHTS) == (1, 2)
    assert [(n, getattr(_abi.TaaParams, n).offset) for n, _ in _abi.TaaParams._fields_] == [("blend", 0), ("jitter", 4), ("previous_jitter", 12), ("flags", 20)]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
OK, INVALID, FORMAT = "well-formed", _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
NAMES = ("lit", "depth", "motion_vectors", "history", "out")
FORMATS = {"lit": RGBA16F, "depth": D32, "motion_vectors": RG16F, "history": RGBA16F, "out": RGBA16F}


def _plane(base, fmt, w, h, pitch=None, ptr=True, offset=0, bpp=None):
    bpp = _abi.FORMAT_BPP[fmt] if bpp is None else bpp
    return _abi.Plane((base + offset) if ptr else None, w, h, w * bpp if pitch is None else pitch, fmt)


def _params(blend=0.1, jitter=(0.25, -0.125), previous_jitter=(-0.25, 0.375), flags=0):
    p = _abi.TaaParams()
    p.blend, p.flags = blend, flags
    p.jitter[:] = jitter
    p.previous_jitter[:] = previous_jitter
    return p


def _cases(base):
    """(name, [lit, depth, motion_vectors, history, out, params], rows, expected)"""
    W, H = 24, 16
    where = {n: base + (i << 16) for i, n in enumerate(NAMES)}

    def call(params=None, **kw):
        p = {n: _plane(where[n], FORMATS[n], W, H) for n in NAMES}
        p.update(kw)
        return [p[n] for n in NAMES] + [_params() if params is None else params]
    yield "whole", call(), (0, 0), OK
    yield "band", call(), (3, 9), OK
    yield "empty band", call(), (5, 5), OK
    yield "hdr weights", call(_params(flags=2)), (0, 0), OK
    yield "blend 1", call(_params(blend=1.0)), (0, 0), OK
    yield "no history, none given", call(_params(flags=1), history=None), (0, 0), OK
    yield "no history, one given but not looked at", call(_params(flags=3), history=_plane(where["history"], D32, 3, 0, ptr=False)), (0, 0), OK
    yield "padded pitches", call(lit=_plane(where["lit"], RGBA16F, W, H, pitch=W * 8 + 4), depth=_plane(where["depth"], D32, W, H, pitch=W * 4 + 12)), (0, 0), OK
    yield "history NULL with a valid history", call(history=None), (0, 0), INVALID
    yield "params NULL", call()[:5] + [None], (0, 0), INVALID
    for n in NAMES:
        fmt, bpp = FORMATS[n], _abi.FORMAT_BPP[FORMATS[n]]
        if n != "history":
            p = call()
            p[NAMES.index(n)] = None
            yield f"{n}: null plane", p, (0, 0), INVALID
        yield f"{n}: null pointer", call(**{n: _plane(where[n], fmt, W, H, ptr=False)}), (0, 0), INVALID
        other = D32 if fmt != D32 else _abi.FORMAT_R32_SFLOAT
        yield f"{n}: wrong format", call(**{n: _plane(where[n], other, W, H, bpp=bpp)}), (0, 0), FORMAT
        yield f"{n}: short pitch", call(**{n: _plane(where[n], fmt, W, H, pitch=W * bpp - 4)}), (0, 0), INVALID
        yield f"{n}: zero width", call(**{n: _plane(where[n], fmt, 0, H)}), (0, 0), INVALID
        yield f"{n}: zero height", call(**{n: _plane(where[n], fmt, W, 0)}), (0, 0), INVALID
        yield f"{n}: other width", call(**{n: _plane(where[n], fmt, W - 1, H)}), (0, 0), INVALID
        yield f"{n}: other height", call(**{n: _plane(where[n], fmt, W, H + 1, pitch=W * bpp)}), (0, 0), INVALID
        yield f"{n}: misaligned pointer", call(**{n: _plane(where[n], fmt, W, H, offset=2)}), (0, 0), INVALID
        yield f"{n}: pitch not a multiple of 4", call(**{n: _plane(where[n], fmt, W, H, pitch=W * bpp + 2)}), (0, 0), INVALID
    yield "lit as R16G16_SFLOAT", call(lit=_plane(where["lit"], RG16F, W, H, bpp=8)), (0, 0), FORMAT
    yield "row_begin > row_end", call(), (9, 3), INVALID
    yield "row_end > H", call(), (0, H + 1), INVALID
    for blend in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        yield f"blend {blend}", call(_params(blend=blend)), (0, 0), INVALID
    for k in range(4):
        for v in (float("nan"), float("inf"), float("-inf")):
            j = [0.25, -0.125, -0.25, 0.375]
            j[k] = v
            yield f"jitter component {k} = {v}", call(_params(jitter=j[:2], previous_jitter=j[2:])), (0, 0), INVALID
    for flags in (4, 8, 0x80000000, 7):
        yield f"flags {flags:#x}", call(_params(flags=flags)), (0, 0), INVALID
    # out's byte range against every input's: the same plane, its last byte on the input's first, its first on the input's last
    size = {n: (H - 1) * W * _abi.FORMAT_BPP[FORMATS[n]] + W * _abi.FORMAT_BPP[FORMATS[n]] for n in NAMES}
    for n in NAMES[:4]:
        yield f"out is {n}'s memory", call(out=_plane(where[n], RGBA16F, W, H)), (0, 0), INVALID
        yield f"out ends inside {n}", call(out=_plane(where[n] - size["out"] + 4, RGBA16F, W, H)), (0, 0), INVALID
        yield f"out begins inside {n}", call(out=_plane(where[n] + size[n] - 4, RGBA16F, W, H)), (0, 0), INVALID
        yield f"out ends where {n} begins", call(out=_plane(where[n] - size["out"], RGBA16F, W, H)), (0, 0), OK
    yield "out is the unread history's memory", call(_params(flags=1), out=_plane(where["history"], RGBA16F, W, H)), (0, 0), OK


def test_every_refusal_of_the_header_on_a_context_without_a_device():
    """A malformed call answers its status; a well-formed one gets as far as selecting the device, which a detached context does not have
    (SAH_ERR_HIP) — so nothing is launched and the made-up addresses are never used."""
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        pytest.skip("a HIP device is present (made-up addresses must not reach a GPU); tests/test_taa_gpu.py checks the refusals there")
    ref_of = lambda a: None if a is None else C.byref(a)  # noqa: E731
    n = 0
    try:
        for name, args, rows, want in _cases(0x10000000):
            got = L.sah_taa_resolve(h, *[ref_of(a) for a in args], *rows)
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"{name}: status {got}"
            n += 1
        ok = next(_cases(0x10000000))[1]
        assert L.sah_taa_resolve(None, *[C.byref(a) for a in ok], 0, 0) == INVALID
    finally:
        L.sah_destroy(h)
    assert n > 90


# ---- the restatement's properties ---------------------------------------------------------------------------------------------------------
def test_history_equal_to_lit_without_motion_is_a_fixed_point():
    """h' == c gives o = c + (c - c) * k = c + 0: the bits of c — for every value but -0, since -0 + +0 = +0 under round to nearest.  So: bit
    for bit on an image with inf and NaN texels and no -0, and on one with -0 channels those, and only those, come out +0."""
    with_zeros, depth, _, _ = ref.random_inputs(37, 23, 5)  # inf, NaN, -0 among the texels
    negative_zero = np.zeros(with_zeros.shape, bool)
    negative_zero[..., :3] = with_zeros[..., :3] == 0x8000
    assert negative_zero.sum() >= 2 and np.isnan(with_zeros.view(np.float16)[..., :3]).any() and np.isinf(with_zeros.view(np.float16)[..., :3]).any()
    lit = np.where(negative_zero, np.uint16(0), with_zeros)
    mv = np.zeros((23, 37, 2), np.uint16)
    for flags in (0, ref.HDR_WEIGHTS):
        for jitter in ((0.0, 0.0), (0.3, -0.2)):
            out, info = ref.resolve_ex(lit, depth, mv, lit, 0.1, jitter, jitter, flags)
            assert out.tobytes() == lit.tobytes()
            assert info["valid"].sum() > 0.9 * info["valid"].size  # (and not because every pixel fell back to lit)
            out, info = ref.resolve_ex(with_zeros, depth, mv, with_zeros, 0.1, jitter, jitter, flags)
            assert out.tobytes() == lit.tobytes() and not info["fallback"][negative_zero.any(-1)].any()


def test_invalid_history_gives_lit():
    lit, depth, mv, history = ref.random_inputs(37, 23, 6)
    for flags in (ref.HISTORY_INVALID, ref.HISTORY_INVALID | ref.HDR_WEIGHTS):
        assert ref.resolve(lit, depth, mv, history, 0.1, (0.1, 0.2), (0.3, 0.4), flags).tobytes() == lit.tobytes()
        assert ref.resolve(lit, depth, mv, None, 0.1, (0.1, 0.2), (0.3, 0.4), flags).tobytes() == lit.tobytes()
    assert ref.resolve(lit, depth, mv, history, 0.1, (0.1, 0.2), (0.3, 0.4), 0).tobytes() != lit.tobytes()


@pytest.mark.parametrize("flags", [0, ref.HDR_WEIGHTS])
def test_finite_output_lies_in_the_neighbourhood_extended_by_the_current_colour(flags):
    lit, depth, mv, history = ref.random_inputs(70, 40, 7, specials=False)
    history = (history.view(np.float16) * np.float16(3.0) - np.float16(2.0)).view(np.uint16)  # far outside the neighbourhood in places
    out, info = ref.resolve_ex(lit, depth, mv, history, 0.25, (0.3, -0.2), (-0.25, 0.4), flags)
    o, c = out.view(np.float16)[..., :3].astype(f32), lit.view(np.float16)[..., :3].astype(f32)
    lo16, hi16 = np.minimum(info["lo"], c).astype(np.float16).astype(f32), np.maximum(info["hi"], c).astype(np.float16).astype(f32)
    assert np.isfinite(o).all() and (o >= lo16).all() and (o <= hi16).all()  # (lo, hi and c are fp16 values: the store's rounding stays inside)
    assert info["clamped"].mean() > 0.2 and (info["valid"] & ~info["clamped"]).any()
    assert (out[..., 3] == lit[..., 3]).all()


def test_min_and_max_ignore_nan_and_order_the_zeros():
    nan, z, nz = f32(np.nan), f32(0.0), f32(-0.0)
    assert ref.fmin(nan, f32(2)) == 2 and ref.fmin(f32(2), nan) == 2 and ref.fmax(nan, f32(2)) == 2 and np.isnan(ref.fmin(nan, nan))
    assert np.signbit(ref.fmin(z, nz)) and np.signbit(ref.fmin(nz, z)) and not np.signbit(ref.fmax(z, nz)) and not np.signbit(ref.fmax(nz, z))
    assert np.signbit(ref.fmax(nz, nz)) and not np.signbit(ref.fmin(z, z))
    lit = np.full((3, 3, 4), np.float16(np.nan)).view(np.uint16)  # a neighbourhood of nothing but NaN keeps the starting values
    lo, hi = ref.neighbourhood(lit)
    assert (lo == np.inf).all() and (hi == -np.inf).all()


def test_dilation_takes_the_first_strictly_nearer_tap_in_tap_order():
    depth = np.full((5, 5), 0.25, f32)
    by, bx = ref.dilated_texel(depth)
    assert (by == np.arange(5)[:, None]).all() and (bx == np.arange(5)[None, :]).all()  # ties: the centre stays
    depth[1, 3] = depth[3, 1] = 0.75  # two equal nearer taps of the centre pixel: (dx, dy) = (1, -1) comes first
    by, bx = ref.dilated_texel(depth)
    assert (by[2, 2], bx[2, 2]) == (1, 3) and (by[0, 0], bx[0, 0]) == (0, 0) and (by[4, 0], bx[4, 0]) == (3, 1)
    depth[2, 2] = np.nan  # a NaN centre is never replaced, and a NaN tap never replaces
    by, bx = ref.dilated_texel(depth)
    assert (by[2, 2], bx[2, 2]) == (2, 2) and (by[2, 3], bx[2, 3]) == (1, 3)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(gen.FIXTURE)


def test_generator_reproduces_the_committed_fixture(fixture):
    got = gen.generate(int(fixture["seed"]))
    assert sorted(got) == sorted(fixture.files)
    for k in fixture.files:
        assert np.asarray(got[k]).dtype == fixture[k].dtype and np.asarray(got[k]).tobytes() == fixture[k].tobytes(), k
    assert fixture["lit"].shape == (ref.TILE[1] + 5, ref.TILE[0] + 5, 4) == (21, 69, 4)
    assert os.path.getsize(gen.FIXTURE) < 200 * 1024


def test_every_planted_case_of_the_fixture_takes_its_branch(fixture):
    fx = fixture
    W, H = 69, 21
    args = (fx["lit"], fx["depth"], fx["motion_vectors"], fx["history"], float(fx["blend"]), fx["jitter"], fx["previous_jitter"])
    plain, info = ref.resolve_ex(*args, 0)
    hdr, _ = ref.resolve_ex(*args, ref.HDR_WEIGHTS)
    assert plain.tobytes() == fx["out_plain"].tobytes() and hdr.tobytes() == fx["out_hdr"].tobytes()
    assert ((plain != hdr).any(-1)).mean() > 0.5
    q, valid, in_range, fallback = info["q"], info["valid"], info["in_range"], info["fallback"]
    # the motion vectors planted in the constant-depth frame are the pixel's own (every tap ties), and land where they were aimed
    by, bx = ref.dilated_texel(fx["depth"])
    for x, y, _, _ in gen.PLANTED_MV:
        assert (by[y, x], bx[y, x]) == (y, x)
    at = {(x, y): (q[y, x, 0], q[y, x, 1]) for x, y, _, _ in gen.PLANTED_MV}
    assert at[(3, 9)][0] == 0 and at[(66, 9)][0] == W and at[(30, 1)][1] == 0 and at[(30, 19)][1] == H
    for x, y in ((3, 9), (66, 9), (30, 1), (30, 19), (5, 12), (64, 5)):  # the boundary itself is inside
        assert in_range[y, x] and valid[y, x] and not fallback[y, x], (x, y)
    assert at[(5, 12)] == (6.5, 12.5)  # a texel centre: the history texel itself, then clamped and blended
    h_at = info["h"][12, 5]
    assert h_at.tobytes() == fx["history"].view(np.float16)[12, 6, :3].astype(f32).tobytes()
    for x, y in ((2, 6), (65, 14)):  # finite, outside
        assert np.isfinite(at[(x, y)]).all() and not in_range[y, x]
    assert np.isinf(at[(4, 15)][0]) and np.isinf(at[(63, 7)][1]) and np.isnan(at[(6, 10)][0]) and np.isnan(at[(62, 11)][1])
    for x, y in ((2, 6), (65, 14), (4, 15), (63, 7), (6, 10), (62, 11)):
        assert fallback[y, x] and (plain[y, x] == fx["lit"][y, x]).all()
    # a history with NaN and inf texels: in range, and refused for the tap's value
    assert (in_range & ~info["history_finite"]).sum() >= 6
    # lit: inf, NaN and -0 are there; a non-finite current colour under a valid history falls back to itself
    lit16 = fx["lit"].view(np.float16)[..., :3]
    assert np.isinf(lit16).sum() >= 2 and np.isnan(lit16).sum() >= 2 and (fx["lit"][..., :3] == 0x8000).sum() >= 2
    assert (valid & fallback).sum() >= 3 and not np.isfinite(lit16[valid & fallback]).all(-1).any()
    finite = np.abs(lit16[np.isfinite(lit16)].astype(f32))
    assert finite.max() > 6e4 and finite[finite != 0].min() < 1e-6  # across the fp16 range
    # -0 decides a bound somewhere: a pixel whose lo or hi is a zero has it with the sign the header's order gives
    assert (np.signbit(info["lo"]) & (info["lo"] == 0)).any()
    # depth: ties with a nearer neighbour (the first in tap order wins), sky, NaN, inf
    d = fx["depth"]
    moved = (by != np.arange(H)[:, None]) | (bx != np.arange(W)[None, :])
    assert moved[5:14, 36:50].any() and (d == 0).sum() >= 40 and np.isnan(d).sum() == 1 and np.isposinf(d).sum() == 1 and np.isneginf(d).sum() == 1
    assert (by[10:13, 32:35] == 11).all() and (bx[10:13, 32:35] == 33).all()  # +inf is the nearest of its neighbourhood
    assert (by[7, 18], bx[7, 18]) == (7, 18)                                   # the NaN centre stays
    # both kinds of valid pixel: the history inside its neighbourhood and clamped to it
    assert info["clamped"].sum() > 100 and (valid & ~info["clamped"]).sum() > 100
    assert (plain[..., 3] == fx["lit"][..., 3]).all() and (hdr[..., 3] == fx["lit"][..., 3]).all()


# ---- the sign of dj ---------------------------------------------------------------------------------------------------------------------------
def test_a_static_cameras_motion_vector_is_jitter_minus_previous_jitter():
    """SceneView twice with different jitters and no motion: the fp64 reprojection of every pixel (tests/mv_reproject.py) is
    jitter - previous_jitter, so mv + (previous_jitter - jitter) is the motion with the jitter taken out: zero."""
    W, H = 64, 36
    j0, j1 = np.array([0.3, -0.2], f32), np.array([-0.25, 0.4], f32)
    v = scene.SceneView.default(W, H)
    v.jitter = j0
    v.update_transforms()
    v.jitter = j1
    v.update_transforms()
    depth = np.random.default_rng(1).uniform(0.001, 0.9, (H, W)).astype(f32)
    mv = mv_reproject.reproject(v.gpu_data, depth)
    want = (j1.astype(np.float64) - j0.astype(np.float64))
    assert np.abs(mv - want).max() < 1e-3, (mv[0, 0], want)
    assert np.abs(want - np.array([-0.55, 0.6])).max() < 1e-6
    # and the restatement reads the history at the pixel's own centre when fed those vectors
    q = ref.history_position(depth, np.broadcast_to(want.astype(np.float16), (H, W, 2)).copy().view(np.uint16), j1, j0)
    centre = np.stack(np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5), -1)
    assert np.abs(q - centre).max() <= 2.0 ** -12 + 1e-6  # half an fp16 spacing below 1


# ---- convergence --------------------------------------------------------------------------------------------------------------------------------
def _stripes(x, y):
    """hard-edged diagonal stripes, 5.3 pixels wide along x: 1.5 or 0.1 at the point (x, y) in pixels"""
    return np.where(np.floor((x + 0.37 * y) / 5.3) % 2 == 0, 1.5, 0.1)


@pytest.mark.parametrize("flags,blend", [(ref.HDR_WEIGHTS, 0.25), (0, 0.25), (ref.HDR_WEIGHTS, 0.1)])
def test_a_static_camera_converges_towards_the_supersampled_image(flags, blend):
    """64 x 36, 32 frames of the façade's 8-phase centred Halton jitter, every frame point-sampled at centre + jitter with
    mv = fp16(jitter - previous_jitter).  Against a 16 x 16 box supersample, the RMSE of each of the last 8 resolved frames is at most 0.75
    of the smallest RMSE any single frame has."""
    W, H, frames = 64, 36, 32
    ys, xs = np.mgrid[0:H, 0:W]
    sub = (np.arange(16) + 0.5) / 16
    truth = _stripes(xs[..., None, None] + sub[None, None, None, :], ys[..., None, None] + sub[None, None, :, None]).mean((-1, -2))
    jitters = ref.jitter_cycle(8)
    depth = np.full((H, W), 0.5, f32)
    single, resolved = [], []
    history, previous = None, None
    for i in range(frames):
        j = jitters[i % 8]
        value = _stripes(xs + 0.5 + float(j[0]), ys + 0.5 + float(j[1]))
        lit = np.stack([value, value, value, np.ones_like(value)], -1).astype(np.float16).view(np.uint16)
        single.append(float(np.sqrt(((value - truth) ** 2).mean())))
        if history is None:
            history = ref.resolve(lit, depth, np.zeros((H, W, 2), np.uint16), None, blend, j, j, flags | ref.HISTORY_INVALID)
        else:
            mv = np.broadcast_to(np.array([j[0] - previous[0], j[1] - previous[1]], f32).astype(np.float16), (H, W, 2)).copy().view(np.uint16)
            history = ref.resolve(lit, depth, mv, history, blend, j, previous, flags)
        previous = j
        got = history.view(np.float16)[..., 0].astype(np.float64)
        resolved.append(float(np.sqrt(((got - truth) ** 2).mean())))
    ratios = [r / min(single) for r in resolved[-8:]]
    print(f"flags {flags}, blend {blend}: single-frame RMSE {min(single):.4f} .. {max(single):.4f}, last 8 resolved / best single {min(ratios):.3f} .. {max(ratios):.3f}")
    assert max(ratios) <= 0.75
