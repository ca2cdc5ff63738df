"""Histogram auto-exposure (include/sah_exposure.h) without a GPU: the exports and the header, the 32- and 16-byte structures, every
refusal the header lists on a context without a device, an argument fuzz in a child process, and the numpy restatement
(tests/exposure_ref.py) — its committed fixture and the properties that make it an exposure meter."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, lib
from tests import exposure_ref as ref
from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_exposure as gen  # noqa: E402

f32 = np.float32
RGBA16F = _abi.FORMAT_R16G16B16A16_SFLOAT
HEADER = os.path.join(ROOT, "include", "sah_exposure.h")
PARAM_FIELDS = ["key", "low_fraction", "high_fraction", "min_exposure", "max_exposure", "adaptation", "max_workgroups", "flags"]
STATE_FIELDS = ["exposure", "adapted", "metered", "window"]


# ---- exports, header, structures ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.EXPOSURE_EXPORTS)
    header = open(HEADER).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.EXPOSURE_EXPORTS) == ["sah_exposure_apply", "sah_exposure_meter"]
    assert not set(lib.EXPOSURE_EXPORTS) & set(lib.EXPORTS)
    hip_h = open(os.path.join(ROOT, "include", "sah_hip.h")).read()
    assert "sah_exposure" not in hip_h and re.search(r"#define\s+SAH_ABI_VERSION\s+6\b", hip_h)  # sah_hip.h's declarations and ABI version stay
    flat = " ".join(header.split())
    assert "ABI-defined" in header and "NOT part of it" in flat and "The result never depends on it" in flat
    assert re.search(r"#define\s+SAH_EXPOSURE_WORK_BYTES\s+1040\b", header) and lib.EXPOSURE_WORK_BYTES == 1040 == 4 * (lib.EXPOSURE_BINS + 4)


@pytest.mark.parametrize("language", ["c", "c++"])
def test_header_compiles_and_the_structures_are_32_and_16_bytes(tmp_path, language):
    src = tmp_path / ("use.c" if language == "c" else "use.cpp")
    check = "_Static_assert" if language == "c" else "static_assert"
    offsets = "".join(f'{check}(offsetof(sah_exposure_params, {n}) == {4 * i}, "{n}");\n' for i, n in enumerate(PARAM_FIELDS))
    offsets += "".join(f'{check}(offsetof(sah_exposure_state, {n}) == {4 * i}, "{n}");\n' for i, n in enumerate(STATE_FIELDS))
    src.write_text('#include <stddef.h>\n#include "sah_exposure.h"\n'
                   f'{check}(sizeof(sah_exposure_params) == 32, "sah_exposure_params");\n{check}(sizeof(sah_exposure_state) == 16, "sah_exposure_state");\n'
                   f'{check}(SAH_EXPOSURE_WORK_BYTES == 4 * (SAH_EXPOSURE_BINS + 4), "work");\n' + offsets +
                   "int use(sah_ctx* c, const sah_plane* p, sah_exposure_state* s, void* w, const sah_exposure_params* q) {\n"
                   "    return sah_exposure_meter(c, p, s, s, w, p, q) + sah_exposure_apply(c, p, s, p, 0, 0) + (int)SAH_EXPOSURE_HISTORY_INVALID; }\n")
    clang = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else "cc"
    subprocess.check_call([clang, "-x", language, "-std=c11" if language == "c" else "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)], timeout=120)
    assert C.sizeof(_abi.ExposureParams) == 32 and C.sizeof(_abi.ExposureState) == 16 == ref.STATE.itemsize
    assert [(n, getattr(_abi.ExposureParams, n).offset) for n, _ in _abi.ExposureParams._fields_] == [(n, 4 * i) for i, n in enumerate(PARAM_FIELDS)]
    assert [(n, getattr(_abi.ExposureState, n).offset) for n, _ in _abi.ExposureState._fields_] == [(n, 4 * i) for i, n in enumerate(STATE_FIELDS)]
    assert list(ref.STATE.names) == STATE_FIELDS
    d = _abi.ExposureParams.default()
    assert {n: getattr(d, n) for n in PARAM_FIELDS} == {k: (f32(v) if isinstance(v, float) else v) for k, v in ref.DEFAULTS.items()}
    assert _abi.ExposureParams.default(adaptation=0.25).adaptation == 0.25 and _abi.EXPOSURE_HISTORY_INVALID == ref.HISTORY_INVALID == 1


def test_adaptation_from_a_frame_time():
    assert frame.adaptation_from(1.0 / 60, 3.0) == pytest.approx(1 - np.exp(-0.05))
    assert 0 < frame.adaptation_from(0.0, 3.0) <= 1 and 0 < frame.adaptation_from(1e-30, 1e-30) <= 1 and frame.adaptation_from(1e9, 1e9) == 1.0
    assert f32(frame.adaptation_from(0.0, 0.0)) > 0  # (0, 1] as an fp32 too


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
OK, INVALID, FORMAT = "well-formed", _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
W, H = 24, 16
SIZE = (H - 1) * W * 8 + W * 8


def _plane(base, w=W, h=H, pitch=None, ptr=True, offset=0, fmt=RGBA16F):
    return _abi.Plane((base + offset) if ptr else None, w, h, w * 8 if pitch is None else pitch, fmt)


def _meter_cases(base):
    """(name, (scene, state_in, state_out, work, exposed_out, params), expected)"""
    scene_at, out_at, work_at, s0, s1 = base, base + (1 << 16), base + (2 << 16), base + (3 << 16), base + (3 << 16) + 64
    P = _abi.ExposureParams.default
    CUT = _abi.EXPOSURE_HISTORY_INVALID

    def call(params="default", **kw):
        a = dict(scene=_plane(scene_at), state_in=s0, state_out=s1, work=work_at, exposed_out=None, params=P() if params == "default" else params)
        a.update(kw)
        return tuple(a[k] for k in ("scene", "state_in", "state_out", "work", "exposed_out", "params"))
    yield "meter only", call(), OK
    yield "fused", call(exposed_out=_plane(out_at)), OK
    yield "fused in place", call(exposed_out=_plane(scene_at)), OK
    yield "one state in place", call(state_in=s1), OK
    yield "a cut without state_in", call(P(flags=CUT), state_in=None), OK
    yield "a cut with a state_in that is not looked at", call(P(flags=CUT), state_in=work_at + 2), OK
    yield "padded pitches", call(scene=_plane(scene_at, pitch=W * 8 + 12), exposed_out=_plane(out_at, pitch=W * 8 + 4)), OK
    yield "limits of the ranges", call(P(low_fraction=0.0, high_fraction=1.0, min_exposure=2.0, max_exposure=2.0, adaptation=1.0, max_workgroups=0xffffffff)), OK
    yield "a tiny adaptation", call(P(adaptation=1e-30, key=1e-30, min_exposure=1e-38, max_exposure=3e38)), OK
    yield "exposed_out ends where the scene begins", call(exposed_out=_plane(scene_at - SIZE)), OK
    yield "work ends where the scene begins", call(work=scene_at - 1040), OK
    for name in ("scene", "state_in", "state_out", "work", "params"):
        yield f"{name} NULL", call(**{name: None}), INVALID
    yield "fused with a cut", call(P(flags=CUT), exposed_out=_plane(out_at)), INVALID
    for n, at in (("scene", scene_at), ("exposed_out", out_at)):
        yield f"{n}: null pointer", call(**{n: _plane(at, ptr=False)}), INVALID
        yield f"{n}: wrong format", call(**{n: _plane(at, fmt=_abi.FORMAT_R32_SFLOAT)}), FORMAT
        yield f"{n}: short pitch", call(**{n: _plane(at, pitch=W * 8 - 4)}), INVALID
        yield f"{n}: misaligned pointer", call(**{n: _plane(at, offset=2)}), INVALID
        yield f"{n}: pitch not a multiple of 4", call(**{n: _plane(at, pitch=W * 8 + 2)}), INVALID
        yield f"{n}: zero width", call(scene=_plane(scene_at, w=0) if n == "scene" else _plane(scene_at), exposed_out=_plane(out_at, w=0)), INVALID
        yield f"{n}: zero height", call(scene=_plane(scene_at, h=0) if n == "scene" else _plane(scene_at), exposed_out=_plane(out_at, h=0)), INVALID
    yield "other width", call(exposed_out=_plane(out_at, w=W - 1)), INVALID
    yield "other height", call(exposed_out=_plane(out_at, h=H + 1)), INVALID
    yield "2^32 texels", call(scene=_plane(scene_at, w=65536, h=65536)), INVALID
    yield "2^31 columns", call(scene=_plane(scene_at, w=2 ** 31, h=1, pitch=0xfffffffc)), INVALID
    for n in ("state_in", "state_out", "work"):
        yield f"{n} misaligned", call(**{n: dict(state_in=s0, state_out=s1, work=work_at)[n] + 2}), INVALID
    nan, inf = float("nan"), float("inf")
    for field in ("key", "min_exposure", "max_exposure"):
        for v in (0.0, -1.0, inf, -inf, nan):
            yield f"{field} {v}", call(P(**{field: v})), INVALID
    yield "min > max", call(P(min_exposure=2.0, max_exposure=1.0)), INVALID
    for lo, hi in ((0.5, 0.5), (0.6, 0.5), (-0.1, 0.5), (0.5, 1.001), (nan, 0.9), (0.1, nan), (-inf, inf)):
        yield f"fractions {lo} .. {hi}", call(P(low_fraction=lo, high_fraction=hi)), INVALID
    for v in (0.0, -0.5, 1.001, inf, nan):
        yield f"adaptation {v}", call(P(adaptation=v)), INVALID
    for flags in (2, 3, 0x80000000):
        yield f"flags {flags:#x}", call(P(flags=flags)), INVALID
    # overlaps: exposed_out against the scene other than the same plane; work and the states against everything
    yield "exposed_out is the scene's memory with another pitch", call(scene=_plane(scene_at, pitch=W * 8 + 8), exposed_out=_plane(scene_at)), INVALID
    yield "exposed_out ends inside the scene", call(exposed_out=_plane(scene_at - SIZE + 4)), INVALID
    yield "exposed_out begins inside the scene", call(exposed_out=_plane(scene_at + SIZE - 4)), INVALID
    yield "state_in half over state_out", call(state_in=s1 + 8), INVALID
    yield "state_in four bytes before state_out", call(state_in=s1 - 4), INVALID
    for n, at in (("work", None), ("state_out", None), ("state_in", None)):
        yield f"{n} begins inside the scene", call(**{n: scene_at + SIZE - 4}), INVALID
        yield f"{n} inside exposed_out", call(exposed_out=_plane(out_at), **{n: out_at + 8}), INVALID
    yield "work ends inside the scene", call(work=scene_at - 1040 + 4), INVALID
    yield "state_out inside work", call(state_out=work_at + 1024), INVALID
    yield "state_in inside work", call(state_in=work_at), INVALID
    yield "state_out ends inside work", call(state_out=work_at - 12), INVALID


def _apply_cases(base):
    """(name, (scene, state, out, row_begin, row_end), expected)"""
    scene_at, out_at, st = base, base + (1 << 16), base + (3 << 16)

    def call(rows=(0, 0), **kw):
        a = dict(scene=_plane(scene_at), state=st, out=_plane(out_at))
        a.update(kw)
        return (a["scene"], a["state"], a["out"]) + tuple(rows)
    yield "whole", call(), OK
    yield "band", call((3, 9)), OK
    yield "empty band", call((5, 5)), OK
    yield "last row", call((H - 1, H)), OK
    yield "in place", call(out=_plane(scene_at)), OK
    yield "out ends where the scene begins", call(out=_plane(scene_at - SIZE)), OK
    for name in ("scene", "state", "out"):
        yield f"{name} NULL", call(**{name: None}), INVALID
    for n, at in (("scene", scene_at), ("out", out_at)):
        yield f"{n}: null pointer", call(**{n: _plane(at, ptr=False)}), INVALID
        yield f"{n}: wrong format", call(**{n: _plane(at, fmt=_abi.FORMAT_D32_SFLOAT)}), FORMAT
        yield f"{n}: short pitch", call(**{n: _plane(at, pitch=W * 8 - 4)}), INVALID
        yield f"{n}: misaligned pointer", call(**{n: _plane(at, offset=2)}), INVALID
        yield f"{n}: pitch not a multiple of 4", call(**{n: _plane(at, pitch=W * 8 + 2)}), INVALID
        yield f"{n}: zero width", call(**{n: _plane(at, w=0)}), INVALID
        yield f"{n}: zero height", call(**{n: _plane(at, h=0)}), INVALID
        yield f"{n}: other width", call(**{n: _plane(at, w=W - 1)}), INVALID
        yield f"{n}: other height", call(**{n: _plane(at, h=H + 1)}), INVALID
    yield "row_begin > row_end", call((9, 3)), INVALID
    yield "row_end > H", call((0, H + 1)), INVALID
    yield "state misaligned", call(state=st + 1), INVALID
    yield "state inside the scene", call(state=scene_at + 16), INVALID
    yield "state inside out", call(state=out_at + SIZE - 4), INVALID
    yield "out is the scene's memory with another pitch", call(scene=_plane(scene_at, pitch=W * 8 + 8), out=_plane(scene_at)), INVALID
    yield "out ends inside the scene", call(out=_plane(scene_at - SIZE + 4)), INVALID
    yield "out begins inside the scene", call(out=_plane(scene_at + SIZE - 4)), INVALID


def test_every_refusal_of_the_header_on_a_context_without_a_device():
    """A malformed call answers its status; a well-formed one gets as far as selecting the device, which a detached context does not have
    (SAH_ERR_HIP) — so nothing is launched and the made-up addresses are never used."""
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        pytest.skip("a HIP device is present (made-up addresses must not reach a GPU); tests/test_exposure_gpu.py checks the refusals there")
    ref_of = lambda a: None if a is None else C.byref(a)  # noqa: E731
    n = 0
    try:
        for name, (scene, s_in, s_out, work, out, params), want in _meter_cases(0x10000000):
            got = L.sah_exposure_meter(h, ref_of(scene), s_in, s_out, work, ref_of(out), ref_of(params))
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"meter, {name}: status {got}"
            n += 1
        for name, (scene, state, out, r0, r1), want in _apply_cases(0x10000000):
            got = L.sah_exposure_apply(h, ref_of(scene), state, ref_of(out), r0, r1)
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"apply, {name}: status {got}"
            n += 1
        scene, s_in, s_out, work, out, params = next(_meter_cases(0x10000000))[1]
        assert L.sah_exposure_meter(None, C.byref(scene), s_in, s_out, work, None, C.byref(params)) == INVALID
        assert L.sah_exposure_apply(None, C.byref(scene), s_in, C.byref(scene), 0, 0) == INVALID
    finally:
        L.sah_destroy(h)
    assert n > 110


@pytest.mark.parametrize("seed", [31, 32])
def test_no_argument_combination_crashes_an_exposure_entry(seed):
    stdout = support.run_fuzz_child("exposure_fuzz_child.py", seed, 2000)
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
    assert (Wf, Hf) == (69, 21) and Wf % ref.TILE[0] and Hf % ref.TILE[1] and Wf % 2 == 1
    assert fixture["scene_plane"].shape == (Hf, gen.PITCH, 4) and (fixture["scene_plane"][:, Wf:] == 0xA5A5).all()
    assert fixture["states"].dtype == ref.STATE and fixture["states"].shape == (3,) and fixture["exposed"].shape == (3, Hf, Wf, 4)
    assert os.path.getsize(gen.FIXTURE) < 64 * 1024


def test_the_fixture_takes_every_branch_it_is_there_for(fixture):
    Wf = gen.WIDTH
    scene = fixture["scene_plane"][:, :Wf]
    L = ref.luminance(scene)
    counted, k = ref.bins_of(L)
    n, states = fixture["histograms"], fixture["states"]
    # uncounted pixels of every kind, both end bins, half denormals
    assert (L == 0).sum() >= 4 and (L < 0).sum() >= 4 and np.isnan(L).sum() >= 4 and np.isposinf(L).sum() >= 2 and np.isneginf(L).sum() >= 2
    assert not counted[(L == 0) | (L < 0) | ~np.isfinite(L)].any() and int(n[0].sum()) == int(counted.sum()) < scene.shape[0] * Wf
    assert n[0][0] >= 3 and n[0][255] >= 2 and (n[0] > 0).sum() > 60
    halfs = scene.view(np.float16)[..., :3]
    assert ((halfs != 0) & (np.abs(halfs) < 6.2e-5)).any(-1).sum() >= 6
    # three metered frames; the gains move the metered value by three octaves and the adaptation follows by a quarter of the way
    assert (states["window"] > 0).all() and (states["metered"] == n[:, 1:].sum(-1)).all()
    alone = [ref.meter(sc, None, dict(gen.PARAMS, flags=ref.HISTORY_INVALID))[1]["adapted"] for sc in gen.frames(scene)]
    assert states["adapted"][0] == alone[0] and abs(float(alone[1] - alone[0]) - 3) < 0.1 and abs(float(alone[2] - alone[0]) + 3) < 0.1
    for i in (1, 2):
        want = states["adapted"][i - 1] + (alone[i] - states["adapted"][i - 1]) * f32(0.25)
        assert states["adapted"][i] == want and states["adapted"][i] != alone[i]
    assert (states["exposure"] > f32(1 / 64)).all() and (states["exposure"] < 64).all()
    # the exposed planes: frame 0 by its own state, frames 1 and 2 by the state before; alpha untouched
    frames = gen.frames(scene)
    for i, used in enumerate([states["exposure"][0], states["exposure"][0], states["exposure"][1]]):
        assert fixture["exposed"][i].tobytes() == ref.apply(frames[i], used).tobytes()
        assert (fixture["exposed"][i][..., 3] == scene[..., 3]).all()


# ---- it is an exposure meter --------------------------------------------------------------------------------------------------------------------
def _constant(L, w=16, h=8):
    """a grey image whose luminance is exactly the fp32 L's nearest grey half (the weights sum to 1 within an ulp)"""
    img = np.zeros((h, w, 4), np.float16)
    img[..., :3] = np.float16(L)
    return img.view(np.uint16)


@pytest.mark.parametrize("L", [2.0 ** -19, 0.001, 0.18, 0.2, 0.99, 1.0, 1.09, 3.7, 100.0, 4000.0])
def test_a_constant_image_is_metered_within_an_eighth_octave_segment(L):
    img = _constant(L)
    lum = float(ref.luminance(img)[0, 0])
    n, st = ref.meter(img, None, dict(low_fraction=0.0, high_fraction=1.0, flags=ref.HISTORY_INVALID, min_exposure=1e-30, max_exposure=1e30))
    assert (n > 0).sum() == 1 and st["metered"] == st["window"] == img.shape[0] * img.shape[1]
    l_avg = float(ref.l_avg_of(st["adapted"]))
    assert 8 / 9 < l_avg / lum < 9 / 8  # bin and centre share one eighth-octave segment
    b = int(np.flatnonzero(n)[0])
    assert b / 8 - 20 <= ref.plog(f32(lum)) < (b + 1) / 8 - 20 and float(st["adapted"]) == (2 * b + 1) / 16 - 20
    assert float(st["exposure"]) == float(f32(0.18) / f32(l_avg))


def test_luminances_beyond_both_ends_fall_into_bins_0_and_255():
    for L, b in ((2.0 ** -21, 0), (6e-8, 0), (2.0 ** -20 * 0.99, 0), (2.0 ** -20, 0), (2.0 ** -20 * 1.1, 1), (3700.0, 254), (3900.0, 255), (2.0 ** 12, 255), (65504.0, 255)):
        n = ref.histogram(_constant(L))
        assert n[b] == 128 and n.sum() == 128, (L, b)
    # bin 0 is counted in the histogram and left out of the average
    img = np.concatenate([_constant(2.0 ** -21), _constant(1.0)])
    n, st = ref.meter(img, None, dict(low_fraction=0.0, high_fraction=1.0, flags=ref.HISTORY_INVALID))
    assert n[0] == 128 and st["metered"] == 128 and float(st["adapted"]) == (2 * 160 + 1) / 16 - 20


def test_no_counted_pixel_gives_clamp_of_one_and_nan_which_the_next_frame_treats_as_no_history():
    img = np.zeros((8, 16, 4), np.float16)
    img[::2, :, 0], img[1::2, ::2, 1], img[1::2, 1::2, 2] = -1.0, np.nan, -np.inf
    img[0, 0, :3] = np.inf
    img = img.view(np.uint16)
    for lo, hi, want in ((1 / 64, 64, 1.0), (2.0, 8.0, 2.0), (0.01, 0.5, 0.5)):
        n, st = ref.meter(img, None, dict(flags=ref.HISTORY_INVALID, min_exposure=lo, max_exposure=hi))
        assert n.sum() == 0 and st["metered"] == 0 and st["window"] == 0 and st["exposure"] == f32(want)
        assert st["adapted"].view(np.uint32) == 0x7fc00000
    # with a history the unmetered frame keeps it
    prev = np.array((0.5, -3.25, 7, 3), ref.STATE)
    _, kept = ref.meter(img, prev)
    assert kept["adapted"] == f32(-3.25) and kept["exposure"] == f32(0.18) / ref.l_avg_of(f32(-3.25))
    # the NaN state is no history for the next frame, flag or no flag
    scene = ref.random_inputs(33, 9, 5)
    _, after_nan = ref.meter(scene, st, dict(adaptation=0.25))
    _, cut = ref.meter(scene, None, dict(adaptation=0.25, flags=ref.HISTORY_INVALID))
    assert after_nan.tobytes() == cut.tobytes() and np.isfinite(cut["adapted"])
    _, still_none = ref.meter(img, st, dict(min_exposure=0.01, max_exposure=0.5))
    assert still_none.tobytes() == st.tobytes()


def test_one_state_in_place_gives_the_bytes_of_the_ping_pong():
    scenes = [ref.random_inputs(40, 12, 70 + i, median=2.0 ** (3 * i - 3)) for i in range(4)]
    s = dict(adaptation=0.25)
    ping = [None, None]
    _, ping[0] = ref.meter(scenes[0], None, dict(s, flags=ref.HISTORY_INVALID))
    _, one = ref.meter(scenes[0], None, dict(s, flags=ref.HISTORY_INVALID))
    trail = [ping[0].tobytes()]
    for i, sc in enumerate(scenes[1:]):
        _, ping[(i + 1) % 2] = ref.meter(sc, ping[i % 2], s)
        _, one = ref.meter(sc, one, s)  # state_out is state_in: read, then written
        assert one.tobytes() == ping[(i + 1) % 2].tobytes()
        trail.append(one.tobytes())
    assert len(set(trail)) == 4


def test_the_result_does_not_depend_on_the_order_of_the_pixels():
    scene = ref.random_inputs(37, 11, 9)
    g = np.random.default_rng(1)
    prev = np.array((1.0, 0.75, 0, 0), ref.STATE)
    n0, s0 = ref.meter(scene, prev, dict(adaptation=0.5))
    for _ in range(3):
        shuffled = g.permutation(scene.reshape(-1, 4)).reshape(11, 37, 4)
        n1, s1 = ref.meter(np.ascontiguousarray(shuffled), prev, dict(adaptation=0.5))
        assert n1.tobytes() == n0.tobytes() and s1.tobytes() == s0.tobytes()
    n2, s2 = ref.meter(np.ascontiguousarray(scene.reshape(11 * 37, 1, 4)), prev, dict(adaptation=0.5))  # another shape of the same pixels
    assert n2.tobytes() == n0.tobytes() and s2.tobytes() == s0.tobytes()


def test_the_window_selects_what_it_says():
    """a single pixel (low and high a hair apart), the whole histogram, and conversions at the ends"""
    n = np.zeros(256, np.uint32)
    n[[10, 100, 200]] = 5, 10, 5
    for lo, hi, bins in ((0.0, 1.0, None), (0.0, 0.25, 10), (0.25, 0.75, 100), (0.75, 1.0, 200), (0.5, 0.55, 100), (0.99, 1.0, None)):
        N, a, b, S = ref.window_sum(n, lo, hi)
        assert N == 20 and (a, b) == (int(f32(20) * f32(lo)), int(f32(20) * f32(hi)))
        if bins is not None:
            assert b > a and S == (b - a) * (2 * bins + 1)
    assert ref.window_sum(n, 0.99, 1.0)[1:3] == (19, 20) and ref.window_sum(n, 0.5, 0.5 + 2.0 ** -20)[1:3] == (10, 10)  # unmetered: hi == lo
    assert ref.f2u(f32(np.nan)) == 0 and ref.f2u(f32(-3)) == 0 and ref.f2u(f32(2.0 ** 32)) == 2 ** 32 - 1 and ref.f2u(f32(7.9)) == 7
    big = np.zeros(256, np.uint32)
    big[255] = 2 ** 32 - 1
    N, a, b, S = ref.window_sum(big, 0.0, 1.0)  # float(N) rounds up to 2^32: f2u saturates and the min brings it back
    assert (N, a, b) == (2 ** 32 - 1, 0, 2 ** 32 - 1) and S == (2 ** 32 - 1) * 511


def test_scale_changes_are_followed_to_within_a_bin():
    """The bound the GPU's frame test relies on: over log-normal images and scale changes of 8, 1/8 and 3, re-metering the exposed image
    gives an exposure within 2^+-0.25 of 1."""
    worst = 0.0
    s = dict(flags=ref.HISTORY_INVALID, min_exposure=1e-6, max_exposure=1e6)
    for seed in range(24):
        base = ref.random_inputs(69, 21, 1000 + seed, median=0.05, sigma=1.5, specials=False)
        for gain in (1.0, 8.0, 0.125, 3.0):
            scene = ref.apply(base, gain)
            _, st = ref.meter(scene, None, s)
            _, again = ref.meter(ref.apply(scene, st["exposure"]), None, s)
            worst = max(worst, abs(float(np.log2(again["exposure"]))))
    print(f"re-metered exposure: 2^{worst:.3f} at most from 1")
    assert worst < 0.25
