"""Screen-space reflections (include/sah_ssr.h) without a GPU: the export and the header, the 36-byte structure and its defaults, every
refusal the header lists on a context without a device, an argument fuzz in a child process, and the numpy restatement (tests/ssr_ref.py) —
its committed fixture, the mirror room's known answer, the monotonicity an exact block skip would rest on, and the condition that the cases
the GPU parity runs over reflect something."""
import collections
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib
from tests import ssr_ref as ref
from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_ssr as gen  # noqa: E402

f32 = np.float32
HEADER = os.path.join(ROOT, "include", "sah_ssr.h")
PARAM_FIELDS = ["max_distance", "thickness", "stride_pixels", "max_steps", "refine_steps", "max_roughness", "edge_fade", "intensity", "flags"]
FORMATS = dict(color=_abi.FORMAT_R8G8B8A8_SRGB, normals=_abi.FORMAT_R16G16B16A16_SFLOAT, data=_abi.FORMAT_R8G8B8A8_UNORM, depth=_abi.FORMAT_D32_SFLOAT,
               source=_abi.FORMAT_R16G16B16A16_SFLOAT, lit=_abi.FORMAT_R16G16B16A16_SFLOAT, scratch=_abi.FORMAT_R32_SFLOAT, out=_abi.FORMAT_R16G16B16A16_SFLOAT)
ORDER = ("color", "normals", "data", "depth", "source", "lit", "scratch", "out")


# ---- exports, header, structure -----------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.SSR_EXPORTS)
    header = open(HEADER).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.SSR_EXPORTS) == ["sah_ssr"]
    assert not set(lib.SSR_EXPORTS) & set(lib.EXPORTS)
    hip_h = open(os.path.join(ROOT, "include", "sah_hip.h")).read()
    assert "sah_ssr" not in hip_h and re.search(r"#define\s+SAH_ABI_VERSION\s+6\b", hip_h)  # sah_hip.h's declarations and ABI version stay
    assert "ABI-defined" in header and "Parity unpinned" in header and "Off by default" in header
    assert "skip" not in header.lower()  # the contract is the plain march; how a kernel may shorten it is DESIGN.md's business
    assert "RESERVED" in header  # scratch: required, checked, not touched
    assert re.search(r"#define\s+SAH_SSR_JITTER\s+1u\b", header) and re.search(r"#define\s+SAH_SSR_REFLECTION_ONLY\s+2u\b", header)
    assert (_abi.SSR_JITTER, _abi.SSR_REFLECTION_ONLY) == (ref.JITTER, ref.REFLECTION_ONLY) == (1, 2)


@pytest.mark.parametrize("language", ["c", "c++"])
def test_header_compiles_and_the_structure_is_36_bytes(tmp_path, language):
    src = tmp_path / ("use.c" if language == "c" else "use.cpp")
    check = "_Static_assert" if language == "c" else "static_assert"
    offsets = "".join(f'{check}(offsetof(sah_ssr_params, {n}) == {4 * i}, "{n}");\n' for i, n in enumerate(PARAM_FIELDS))
    src.write_text('#include <stddef.h>\n#include "sah_ssr.h"\n'
                   f'{check}(sizeof(sah_ssr_params) == 36, "sah_ssr_params");\n' + offsets +
                   "int use(sah_ctx* c, const sah_view_data* v, const sah_plane* p, const sah_ssr_params* q) {\n"
                   "    return sah_ssr(c, v, p, p, p, p, p, p, p, p, q, 0, 0) + (int)(SAH_SSR_JITTER | SAH_SSR_REFLECTION_ONLY); }\n")
    clang = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else "cc"
    subprocess.check_call([clang, "-x", language, "-std=c11" if language == "c" else "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)], timeout=120)
    assert C.sizeof(_abi.SsrParams) == 36
    assert [(n, getattr(_abi.SsrParams, n).offset) for n, _ in _abi.SsrParams._fields_] == [(n, 4 * i) for i, n in enumerate(PARAM_FIELDS)]


def test_the_headers_defaults_are_the_python_defaults():
    header = open(HEADER).read()
    d = _abi.SsrParams.default()
    for name in PARAM_FIELDS[:-1]:
        m = re.search(rf"#define\s+SAH_SSR_DEFAULT_{name.upper()}\s+([0-9.]+)[fu]\b", header)
        assert m, name
        assert f32(float(m.group(1))) == f32(getattr(d, name)) == f32(ref.DEFAULTS[name]), name
        assert re.search(rf"{name};[^\n]*default {re.escape(m.group(1).rstrip('0').rstrip('.'))}\b", header), name  # the field's comment says the same
    assert d.flags == 0 == ref.DEFAULTS["flags"]
    assert _abi.SsrParams.default(stride_pixels=2.5, flags=3).stride_pixels == 2.5 and _abi.SsrParams.default(flags=3).flags == 3


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
OK, INVALID, FORMAT = "well-formed", _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
W, H = 24, 18
SW, SH = 3, 3  # the scratch plane: ceil(W / 8) x ceil(H / 8)


def _plane(name, base, w=None, h=None, pitch=None, ptr=True, offset=0, fmt=None):
    bpp = _abi.FORMAT_BPP[FORMATS[name]]
    w = (SW if name == "scratch" else W) if w is None else w
    h = (SH if name == "scratch" else H) if h is None else h
    return _abi.Plane((base + offset) if ptr else None, w, h, w * bpp if pitch is None else pitch, FORMATS[name] if fmt is None else fmt)


def _view(**changes):
    v = _abi.ViewData()
    for i in (0, 5, 10, 15):
        v.view[i] = 1.0
    v.projection[0], v.projection[5], v.projection[8], v.projection[9], v.projection[11], v.z_near = 1.0, 1.7, 0.01, -0.02, -1.0, 0.05
    for k, val in changes.items():
        if k == "z_near":
            v.z_near = val
        elif k.startswith("projection"):
            v.projection[int(k[10:])] = val
        else:
            v.view[int(k[4:])] = val
    return v


def _cases(base):
    """(name, (view, planes by name, params, row_begin, row_end), expected)"""
    at = {n: base + (i << 16) for i, n in enumerate(ORDER)}
    P = _abi.SsrParams.default
    size8 = (H - 1) * W * 8 + W * 8

    def call(rows=(0, 0), params="default", view="default", **kw):
        planes = {n: _plane(n, at[n]) for n in ORDER}
        planes.update(kw)
        return (_view() if view == "default" else view, planes, P() if params == "default" else params) + tuple(rows)
    yield "whole", call(), OK
    yield "band", call((3, 9)), OK
    yield "empty band", call((5, 5)), OK
    yield "last row", call((H - 1, H)), OK
    yield "lit is source", call(lit=_plane("lit", at["source"])), OK
    yield "padded pitches", call(lit=_plane("lit", at["lit"], pitch=W * 8 + 12), out=_plane("out", at["out"], pitch=W * 8 + 4),
                                 scratch=_plane("scratch", at["scratch"], pitch=SW * 4 + 8)), OK
    yield "limits of the ranges", call(params=P(thickness=0.0, stride_pixels=1.0, max_steps=1, refine_steps=0, max_roughness=1.0, edge_fade=0.5, intensity=0.0,
                                                flags=3)), OK
    yield "other limits", call(params=P(thickness=float("inf"), max_steps=256, refine_steps=8, max_roughness=1e-6, edge_fade=1e-6, max_distance=3e38)), OK
    yield "out ends where lit begins", call(out=_plane("out", at["lit"] - size8)), OK
    for name in ORDER:
        yield f"{name} NULL", call(**{name: None}), INVALID
        yield f"{name}: null pointer", call(**{name: _plane(name, at[name], ptr=False)}), INVALID
        other = _abi.FORMAT_R32_SFLOAT if FORMATS[name] != _abi.FORMAT_R32_SFLOAT else _abi.FORMAT_D32_SFLOAT
        yield f"{name}: wrong format", call(**{name: _plane(name, at[name], fmt=other)}), FORMAT
        bpp = _abi.FORMAT_BPP[FORMATS[name]]
        w = SW if name == "scratch" else W
        yield f"{name}: short pitch", call(**{name: _plane(name, at[name], pitch=w * bpp - 4)}), INVALID
        yield f"{name}: misaligned pointer", call(**{name: _plane(name, at[name], offset=2)}), INVALID
        yield f"{name}: pitch not a multiple of 4", call(**{name: _plane(name, at[name], pitch=w * bpp + 2)}), INVALID
        yield f"{name}: zero width", call(**{name: _plane(name, at[name], w=0)}), INVALID
        yield f"{name}: zero height", call(**{name: _plane(name, at[name], h=0)}), INVALID
        yield f"{name}: other width", call(**{name: _plane(name, at[name], w=w + 1, pitch=(w + 1) * bpp)}), INVALID
        yield f"{name}: other height", call(**{name: _plane(name, at[name], h=(SH if name == "scratch" else H) - 1)}), INVALID
    yield "scratch of the frame's extent", call(scratch=_plane("scratch", at["scratch"], w=W, h=H)), INVALID
    yield "view NULL", call(view=None), INVALID
    yield "params NULL", call(params=None), INVALID
    yield "row_begin > row_end", call((9, 3)), INVALID
    yield "row_end > H", call((0, H + 1)), INVALID
    nan, inf = float("nan"), float("inf")
    bad = dict(max_distance=(0.0, -1.0, inf, nan), thickness=(-0.001, -inf, nan), stride_pixels=(0.999, 0.0, -4.0, inf, nan), max_steps=(0, 257, 0xFFFFFFFF),
               refine_steps=(9, 0xFFFFFFFF), max_roughness=(0.0, -0.5, 1.001, inf, nan), edge_fade=(0.0, -0.1, 0.501, inf, nan), intensity=(-0.001, inf, nan),
               flags=(4, 7, 0x80000000))
    for field, values in bad.items():
        for v in values:
            yield f"{field} {v}", call(params=P(**{field: v})), INVALID
    for field in ("projection0", "projection5", "projection8", "projection9", "z_near", "view0", "view1", "view2", "view4", "view5", "view6", "view8", "view9", "view10"):
        yield f"view: {field} NaN", call(view=_view(**{field: nan})), INVALID
    for v in (0.0, -0.05, inf):
        yield f"z_near {v}", call(view=_view(z_near=v)), INVALID
    yield "view: a field the pass does not read is NaN", call(view=_view(view12=nan, projection10=nan)), OK
    # overlaps
    for name in ORDER[:-1]:
        yield f"out is {name}'s memory", call(out=_plane("out", at[name])), INVALID
    yield "out ends inside lit", call(out=_plane("out", at["lit"] - size8 + 4)), INVALID
    yield "out begins inside source", call(out=_plane("out", at["source"] + size8 - 4)), INVALID
    for name in ORDER[:6]:
        yield f"scratch is {name}'s memory", call(scratch=_plane("scratch", at[name])), INVALID


def _invoke(L, h, args):
    view, planes, params, r0, r1 = args
    ref_of = lambda a: None if a is None else C.byref(a)  # noqa: E731
    return L.sah_ssr(h, ref_of(view), *[ref_of(planes[n]) for n in ORDER], ref_of(params), r0, r1)


def test_every_refusal_of_the_header_on_a_context_without_a_device():
    """A malformed call answers its status; a well-formed one gets as far as selecting the device, which a detached context does not have
    (SAH_ERR_HIP) — so nothing is launched and the made-up addresses are never used."""
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        pytest.skip("a HIP device is present (made-up addresses must not reach a GPU); tests/test_ssr_gpu.py checks the refusals there")
    n = 0
    try:
        for name, args, want in _cases(0x10000000):
            got = _invoke(L, h, args)
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"{name}: status {got}"
            n += 1
        assert _invoke(L, None, next(_cases(0x10000000))[1]) == INVALID
    finally:
        L.sah_destroy(h)
    assert n > 150


@pytest.mark.parametrize("seed", [43])
def test_no_argument_combination_crashes_the_entry(seed):
    stdout = support.run_fuzz_child("ssr_fuzz_child.py", seed, 2000)
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
    assert (gen.WIDTH, gen.HEIGHT) == (96, 54) and gen.HEIGHT % ref.BLOCK and gen.HEIGHT % ref.TRACE_TILE[1]
    assert fixture["out"].shape == (len(gen.CASES), gen.HEIGHT, gen.WIDTH, 4)
    assert os.path.getsize(gen.FIXTURE) < 256 * 1024


def test_the_fixture_takes_every_branch_it_is_there_for(fixture):
    frame = {k: fixture[k] for k in gen.PLANES}
    seen = collections.Counter()
    for i, params in enumerate(gen.CASES):
        out, info = ref.ssr_ex(view=gen.view(), params=params, **frame)
        assert out.tobytes() == fixture["out"][i].tobytes()
        seen.update(info["outcome"].ravel().tolist())
        hit = info["hit"]
        if params.get("flags", 0) & ref.REFLECTION_ONLY:
            assert (out[~hit] == 0).all() and (out[hit][:, 3] != 0).any()
        else:
            assert (out[~hit] == frame["lit"][~hit]).all() and (out[..., 3] == frame["lit"][..., 3]).all()
            assert (out[hit][:, :3] != frame["lit"][hit][:, :3]).any(-1).mean() > 0.8
        if i == 0:
            assert hit[:, :gen.SPLIT].mean() > 0.1 and info["refined"].sum() > 100
            rejected = info["outcome"] == ref.REJECTED
            unclean = {(x, y) for x, y, _, _ in gen.UNCLEAN}
            assert unclean <= {(int(x), int(y)) for x, y in zip(info["hx"][rejected], info["hy"][rejected])}  # each planted texel was some ray's hit
    assert len({fixture["out"][i].tobytes() for i in range(len(gen.CASES))}) == len(gen.CASES)
    assert all(seen[k] > 0 for k in ref.OUTCOMES if k != ref.NO_INTENSITY), {ref.OUTCOMES[k]: seen[k] for k in ref.OUTCOMES}


# ---- the mirror room: a known answer ---------------------------------------------------------------------------------------------------------
def test_a_floor_pixel_sees_the_wall_where_geometry_says():
    w, h = 96, 54
    frame, masks = ref.mirror_room(w, h)
    worst = {}
    thick = 3e38  # a wall as thick as can be: the hit is the first sample at or behind it, whichever that is, so its row depends on the stride
    for stride in (4.0, 2.0, 1.0):
        out, info = ref.ssr_ex(view=ref.room_view(), params=dict(thickness=thick, stride_pixels=stride, max_steps=256, refine_steps=0), **frame)
        hit = info["hit"] & masks["floor"]
        assert hit.sum() > 0.1 * w * h and masks["wall"][info["hy"][hit], info["hx"][hit]].all()  # a floor pixel's hit lies on the wall
        ys, xs = np.nonzero(hit)
        want = np.array([ref.mirror_row(y, h) for y in ys])
        # the ray runs up the image: its hit is the first sample at or behind the wall, so at most one stride beyond the mirror image
        err = np.abs((info["hy"][hit] + 0.5) - want)
        assert err.max() <= stride, (stride, err.max())
        worst[stride] = {(int(y), int(x)): float(e) for y, x, e in zip(ys, xs, err)}
        # the reflection is the wall's stripe: out - lit is the weight times the stripe's colour, red and green a fixed multiple of blue's row code
        src = frame["source"][info["hy"][hit], info["hx"][hit]]
        assert (src[:, 3] == np.float16(1.0).view(np.uint16)).all()
    for fine, coarse in ((2.0, 4.0), (1.0, 2.0)):  # halving the stride never moves a hit further from the mirror image
        common = set(worst[fine]) & set(worst[coarse])
        assert len(common) > 500 and all(worst[fine][p] <= worst[coarse][p] for p in common)
    assert sum(worst[2.0][p] < worst[4.0][p] for p in set(worst[2.0]) & set(worst[4.0])) > 500  # and from 4 to 2 it brings many of them closer
    # refinement pulls the hit to the crossing: with 8 bisections every hit is within a texel of the mirror image
    out, info = ref.ssr_ex(view=ref.room_view(), params=dict(thickness=thick, stride_pixels=4.0, max_steps=256, refine_steps=8), **frame)
    hit = info["hit"] & masks["floor"]
    want = np.array([ref.mirror_row(y, h) for y in np.nonzero(hit)[0]])
    assert np.abs((info["hy"][hit] + 0.5) - want).max() <= 1.0
    # sky and the rough wall pass through
    assert (out[~masks["floor"]] == frame["lit"][~masks["floor"]]).all()


# ---- what a block skip would rest on -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, ref.JITTER])
def test_the_rays_depth_and_texel_are_monotone_in_the_sample_index(flags):
    """zr_i, and each texel coordinate, never turns round along a ray — for random rays of random G-buffers, a long max_distance included"""
    for (w, h, seed, dist, stride) in ((65, 33, 1, 50.0, 1.0), (192, 48, 2, 1.0e6, 2.5), (40, 40, 3, 3.0, 4.0)):
        frame, view = ref.random_frame(w, h, seed), ref.random_view(w, h)
        p = dict(ref.DEFAULTS, max_distance=dist, stride_pixels=stride, flags=flags)
        with np.errstate(all="ignore"):
            surface, z = ref.linear_depth(frame["depth"], view.z_near)
            rays = ref.Rays(ref.positions(z, view, w, h), z, ref.view_normals(frame["normals"], view), view, w, h, p)
            live = surface & rays.ok
            assert live.sum() > 0.5 * w * h
            prev, up, down = None, np.zeros((h, w), bool), np.zeros((h, w), bool)
            xdir, ydir = np.sign(rays.dsx), np.sign(rays.dsy)
            for i in range(1, 257):
                t = rays.t_of(i)
                inside, ix, iy, zr = rays.sample(t)
                cur = live & (t <= 1) & inside
                assert (zr[cur] > 0).all()
                if prev is not None:
                    both = cur & prev[0]
                    up |= both & (zr > prev[1])
                    down |= both & (zr < prev[1])
                    assert ((ix - prev[2])[both] * xdir[both] >= 0).all() and ((iy - prev[3])[both] * ydir[both] >= 0).all()
                prev = (cur, zr, ix, iy)
            assert not (up & down).any() and up.sum() > 100 and down.sum() > 100


# ---- the coverage condition of the GPU parity ----------------------------------------------------------------------------------------------------
def test_the_gpu_parity_cases_reflect_something_and_take_every_outcome():
    """A condition, not a measurement: over the cases tests/test_ssr_gpu.py compares with the restatement there is at least one pixel of every
    outcome, with "behind" samples and refined hits, and the mirror-room cases have at least a tenth of their pixels hitting."""
    seen = collections.Counter()
    behind = refined = 0
    names = []
    for name, frame, view, settings in ref.parity_cases():
        names.append(name)
        out, info = ref.ssr_ex(view=view, params=settings, **frame)
        seen.update(info["outcome"].ravel().tolist())
        behind += int((info["behind"] > 0).sum())
        refined += int(info["refined"].sum())
        if name.startswith("room"):
            assert info["hit"].mean() >= 0.1, name
        if name.startswith("far"):
            traced = np.isin(info["outcome"], (ref.MISS_T, ref.MISS_IMAGE, ref.MISS_STEPS, ref.REJECTED, ref.HIT))
            assert (info["outcome"] == ref.MISS_IMAGE).sum() > 0.5 * traced.sum(), name  # most of the rays that are marched leave the image
    assert len(names) == len(set(names)) == len(ref.EXTENTS) * len(ref.RANDOM_SETTINGS) + 3
    assert {(8, 8), (7, 9), (9, 7), (31, 7), (32, 8), (33, 9)} <= set(ref.EXTENTS)  # around the block and the trace kernel's tile
    out, info = ref.ssr_ex(view=ref.room_view(), params=dict(ref.ROOM_SETTINGS, intensity=0.0), **ref.mirror_room(48, 27)[0])
    seen.update(info["outcome"].ravel().tolist())  # (the identity test's case)
    assert all(seen[k] > 0 for k in ref.OUTCOMES), {ref.OUTCOMES[k]: seen[k] for k in ref.OUTCOMES}
    assert behind > 0 and refined > 0
