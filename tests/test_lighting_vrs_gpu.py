"""GPU: sah_lighting_vrs and sah_vrsaa_resolve (include/sah_vrs.h).  The contract of the first is a gather: with `full` what sah_lighting
writes for the same descriptor and (sy, sx) the source map of the numpy restatement (tests/lighting_vrs_ref.py), the call must write
full[sy, sx] — 0 differing bytes.  The inputs are util.LightingFrame's with the depth planes tests/test_lighting_vrs_cpu.py shows to
exercise every class of the map; `full` of one case is compared with the oracle here, which closes the chain.  The kernel's region is
32 x 32 pixels, four adjacent pixels of a row per thread."""
import ctypes as C
import faulthandler
import functools
import os
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, images, lib
from tests import lighting_vrs_ref as ref
from tests import util
from tests.support import context_state, differs, Image, SENTINEL, side_stream_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_vrs as gen  # noqa: E402

RGBA16F = _abi.FORMAT_R16G16B16A16_SFLOAT
PATTERN = 0x0101 * SENTINEL  # what every half of an untouched output plane holds
SUNS = [_abi.SHADOW_MODE_OFF, _abi.SHADOW_MODE_CSM, _abi.SHADOW_MODE_RT]
GIS = [_abi.GI_NONE, _abi.GI_LPV]
FORMATS = {"color": _abi.FORMAT_R8G8B8A8_SRGB, "normals": RGBA16F, "data": _abi.FORMAT_R8G8B8A8_UNORM, "emission": _abi.FORMAT_R8G8B8A8_SRGB,
           "depth": _abi.FORMAT_D32_SFLOAT, "ao": _abi.FORMAT_R32_SFLOAT, "shadow_mask": _abi.FORMAT_R32_SFLOAT}


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)  # each test under a limit of its own: an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


class Case:
    """one parity case under one sun mode and GI kind: the frame, its device arrays, what sah_lighting writes (computed once) and the map"""

    def __init__(self, ctx, case, sun, gi):
        self.w, self.h, self.texel = ref.PARITY_CASES[case]
        self.depth, self.rates = ref.parity_inputs(case)
        self.f = util.LightingFrame(self.w, self.h, seed=31 + case, sun_mode=sun, gi=gi, sky=True)
        self.f.arrays["depth"] = self.depth
        self.dev = self.f.device_arrays()
        self.full = self.f.run_hip(ctx, self.dev)
        self.full.setflags(write=False)
        self.sy, self.sx = ref.source_map(self.depth, self.rates, self.texel, ref.TOLERANCE)

    def want(self, rates=None, tol=ref.TOLERANCE):
        sy, sx = (self.sy, self.sx) if rates is None and tol == ref.TOLERANCE else ref.source_map(self.depth, rates if rates is not None else self.rates, self.texel, tol)
        return self.full[sy, sx]

    def run(self, ctx, rates=None, tol=ref.TOLERANCE, rows=(0, 0)):
        """sah_lighting_vrs over tight device arrays into a plane of PATTERN: its texels"""
        import torch
        lit = torch.full((self.h, self.w, 4), PATTERN - 0x10000, dtype=torch.int16, device="cuda")
        sri = util.to_torch(np.ascontiguousarray(self.rates if rates is None else rates))
        self.f.row_begin, self.f.row_end = rows
        try:
            d, keep = self.f.describe(self.dev, lit)
        finally:
            self.f.row_begin = self.f.row_end = 0
        ctx.lighting_vrs(d, images.plane(sri, _abi.FORMAT_R8_UINT), self.texel, tol)
        torch.cuda.synchronize()
        return util.from_torch(lit, np.uint16)


@functools.lru_cache(maxsize=None)
def _case(ctx, case, sun, gi):
    return Case(ctx, case, sun, gi)


# ---- parity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gi", GIS)
@pytest.mark.parametrize("sun", SUNS)
@pytest.mark.parametrize("case", range(len(ref.PARITY_CASES)))
def test_parity_with_the_gather_of_sah_lighting(hip_ctx, case, sun, gi):
    c = _case(hip_ctx, case, sun, gi)
    got = c.run(hip_ctx)
    want = c.want()
    assert got.tobytes() == want.tobytes(), f"case {ref.PARITY_CASES[case]}, sun {sun}, gi {gi}: " + differs(got, want)
    assert (got != c.full).any(), "the gather is not the identity: the variable-rate frame differs from the full-rate one"
    assert c.run(hip_ctx).tobytes() == got.tobytes()  # repeatable


def test_the_full_rate_frame_is_the_oracles(hip_ctx):
    """the other half of the chain: `full`, which every comparison above gathers from, against the CPU oracle"""
    c = _case(hip_ctx, 0, _abi.SHADOW_MODE_CSM, _abi.GI_LPV)
    d = util.f16_ulp_diff(c.full, c.f.run_oracle())
    print(util.report_ulp("sah_lighting on the first parity case, CSM + LPV + sky", d))
    assert int(d.max()) <= util.MAX_ULP


@pytest.mark.parametrize("sun,gi", [(_abi.SHADOW_MODE_CSM, _abi.GI_LPV), (_abi.SHADOW_MODE_RT, _abi.GI_NONE)])
def test_uniform_1x1_is_sah_lighting(hip_ctx, sun, gi):
    for case in (0, 1):
        c = _case(hip_ctx, case, sun, gi)
        for code in (0, 0xf0):
            got = c.run(hip_ctx, np.full_like(c.rates, code), float("inf"))
            assert got.tobytes() == c.full.tobytes(), differs(got, c.full)


def test_tolerances_zero_and_infinite(hip_ctx):
    c = _case(hip_ctx, 0, _abi.SHADOW_MODE_CSM, _abi.GI_LPV)
    fx = np.load(gen.FIXTURE)
    assert np.array_equal(fx["depth"].view(np.uint32), c.depth.view(np.uint32)) and np.array_equal(fx["rate_image"], c.rates)
    for tol, (sy, sx) in zip(fx["tolerances"], fx["source_map"]):
        got = c.run(hip_ctx, tol=float(tol))
        want = c.full[sy.astype(np.int64), sx.astype(np.int64)]
        assert got.tobytes() == want.tobytes(), f"tolerance {tol}: " + differs(got, want)


def test_uniform_coarse_rates(hip_ctx):
    """every code of a uniform image that names another rate, 1 x 4 and 4 x 1 (which the VRSAA pass never stores) included"""
    c = _case(hip_ctx, 0, _abi.SHADOW_MODE_RT, _abi.GI_LPV)
    for code in (1, 2, 4, 5, 6, 8, 9, 10, 0x0f, 0x3b):
        rates = np.full_like(c.rates, code)
        got = c.run(hip_ctx, rates, float("inf"))
        want = c.want(rates, float("inf"))
        assert got.tobytes() == want.tobytes(), f"code {code}: " + differs(got, want)


def test_force_general_gives_the_same_bytes(hip_ctx):
    c = _case(hip_ctx, 1, _abi.SHADOW_MODE_CSM, _abi.GI_LPV)
    assert c.f.run_hip(hip_ctx, c.dev).tobytes() == c.full.tobytes()
    hip_ctx.debug_set(force_general=True)
    try:
        assert c.f.run_hip(hip_ctx, c.dev).tobytes() == c.full.tobytes() and hip_ctx.lighting_dispatch()["family"] == "general"
        got = c.run(hip_ctx)
    finally:
        hip_ctx.debug_set()
    assert got.tobytes() == c.want().tobytes()


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
class Planes:
    """the planes of a case, each with a pitch and an offset of its own, guard bytes around every one: pad in texels, offset in texels"""

    def __init__(self, c, pad, offset, rate_extra):
        a = c.f.arrays
        self.inputs = {k: Image(fmt, c.w, c.h, (c.w + pad) * _abi.FORMAT_BPP[fmt], a[k], offset * _abi.FORMAT_BPP[fmt]) for k, fmt in FORMATS.items() if k in a}
        self.lit = Image(RGBA16F, c.w, c.h, (c.w + pad) * 8, None, offset * 8)
        sh, sw = c.rates.shape
        wide = np.full((sh + 1, sw + rate_extra), 10, np.uint8)  # larger than needed: accepted, the extra texels never read for a pixel
        wide[:sh, :sw] = c.rates
        self.rate = Image(_abi.FORMAT_R8_UINT, sw + rate_extra, sh + 1, sw + rate_extra + 5, wide, 3)

    def describe(self, c, rows=(0, 0)):
        import torch
        d, keep = c.f.describe(c.dev, torch.zeros((1, 1, 4), dtype=torch.int16, device="cuda"))  # (the uniform blocks, volumes and LUTs; every plane is replaced below)
        gb = _abi.GBuffer(*(self.inputs[k].plane for k in ("color", "normals", "data", "emission", "depth")))
        d.gbuffer, d.lit, d.ao = C.pointer(gb), C.pointer(self.lit.plane), C.pointer(self.inputs["ao"].plane)
        if "shadow_mask" in self.inputs:
            d.shadow_mask = C.pointer(self.inputs["shadow_mask"].plane)
        d.row_begin, d.row_end = rows
        return d, keep + [gb]

    def texels(self):
        return self.lit.texels(np.uint16).reshape(self.lit.h, self.lit.w, 4)

    def inputs_unchanged(self):
        return all(i.unchanged() for i in self.inputs.values()) and self.rate.unchanged()


# 64 x 36: 16-byte rows on 16-byte bases take the kernel's 16-byte accesses, the other layout its scalar ones at the same width; 75 x 45 odd
@pytest.mark.parametrize("case,pad,offset", [(1, 4, 4), (1, 1, 1), (0, 3, 2)])
@pytest.mark.parametrize("sun,gi", [(_abi.SHADOW_MODE_CSM, _abi.GI_LPV), (_abi.SHADOW_MODE_RT, _abi.GI_NONE)])
def test_pitched_offset_planes_sentinels_and_inputs(hip_ctx, case, pad, offset, sun, gi):
    import torch
    c = _case(hip_ctx, case, sun, gi)
    p = Planes(c, pad, offset, rate_extra=2)
    d, keep = p.describe(c)
    hip_ctx.lighting_vrs(d, p.rate.plane, c.texel, ref.TOLERANCE)
    torch.cuda.synchronize()
    got, want = p.texels(), c.want()
    assert got.tobytes() == want.tobytes(), differs(got, want)
    assert p.lit.padding_intact(), "bytes outside the texels of lit changed"
    assert p.inputs_unchanged()


@pytest.mark.parametrize("rows", [(8, 28), (40, 45), (0, 4), (44, 45), (12, 12)])
def test_row_bands(hip_ctx, rows):
    import torch
    c = _case(hip_ctx, 0, _abi.SHADOW_MODE_CSM, _abi.GI_LPV)
    assert c.h == 45
    p = Planes(c, 1, 1, rate_extra=0)
    d, keep = p.describe(c, rows)
    hip_ctx.lighting_vrs(d, p.rate.plane, c.texel, ref.TOLERANCE)
    torch.cuda.synchronize()
    got, want = p.texels(), np.full((c.h, c.w, 4), PATTERN, np.uint16)
    want[rows[0]:rows[1]] = c.want()[rows[0]:rows[1]]  # the whole-frame call on the band's rows, the sentinel elsewhere
    assert got.tobytes() == want.tobytes(), f"rows {rows}: " + differs(got, want)
    assert p.lit.padding_intact(rows) and p.inputs_unchanged()
    assert c.run(hip_ctx, rows=rows).tobytes() == want.tobytes()


def test_no_side_effects_on_the_context(hip_ctx):
    c = _case(hip_ctx, 1, _abi.SHADOW_MODE_CSM, _abi.GI_LPV)
    c.f.run_hip(hip_ctx, c.dev)

    def state():
        return context_state(hip_ctx)
    before = state()
    got = c.run(hip_ctx)
    assert state() == before
    assert got.tobytes() == c.want().tobytes()
    assert c.f.run_hip(hip_ctx, c.dev).tobytes() == c.full.tobytes()  # and sah_lighting goes on as before


def test_recorded_under_stream_capture_and_replayed(hip_ctx):
    import torch
    c = _case(hip_ctx, 0, _abi.SHADOW_MODE_CSM, _abi.GI_LPV)
    with side_stream_context() as (ctx, s):
        lit = torch.full((c.h, c.w, 4), PATTERN - 0x10000, dtype=torch.int16, device="cuda")
        sri = util.to_torch(c.rates)
        d, keep = c.f.describe(c.dev, lit)
        sri_p = images.plane(sri, _abi.FORMAT_R8_UINT)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ctx.lighting_vrs(d, sri_p, c.texel, ref.TOLERANCE)
        torch.cuda.synchronize()
        assert (util.from_torch(lit, np.uint16) == PATTERN).all()  # recorded, not run
        rates2 = np.roll(c.rates, 3, axis=1)  # replayed over another image in the same memory
        sri.copy_(util.to_torch(np.ascontiguousarray(rates2)))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got, want = util.from_torch(lit, np.uint16), c.want(rates2)
        assert got.tobytes() == want.tobytes(), differs(got, want)
        assert want.tobytes() != c.want().tobytes()


# ---- the resolve --------------------------------------------------------------------------------------------------------------------------
def _resolve(ctx, lit_np, pitches=(None, None), offsets=(0, 0), rows=(0, 0)):
    import torch
    h2, w2 = lit_np.shape[:2]
    w, h = w2 // 2, h2 // 2
    lit = Image(RGBA16F, w2, h2, pitches[0], lit_np, offsets[0])
    out = Image(RGBA16F, w, h, pitches[1], None, offsets[1])
    ctx.vrsaa_resolve(lit.plane, out.plane, rows)
    torch.cuda.synchronize()
    got = out.texels(np.uint16).reshape(h, w, 4)
    r0, r1 = (0, h) if tuple(rows) == (0, 0) else rows
    want = np.full((h, w, 4), PATTERN, np.uint16)
    want[r0:r1] = ref.resolve(lit_np, rows)
    assert got.tobytes() == want.tobytes(), f"{w} x {h}, pitches {pitches}, offsets {offsets}, rows {rows}: " + differs(got, want)
    assert out.padding_intact((r0, r1)) and lit.unchanged()
    return got


# 37 x 21: scalar accesses; 64 x 36: 16-byte accesses on aligned planes, scalar ones on the others
@pytest.mark.parametrize("extent,pitches,offsets", [((37, 21), (None, None), (0, 0)), ((37, 21), (74 * 8 + 8, 37 * 8 + 24), (8, 24)),
                                                    ((64, 36), (None, None), (0, 0)), ((64, 36), (128 * 8 + 64, 64 * 8 + 32), (16, 32)),
                                                    ((64, 36), (128 * 8 + 8, 64 * 8), (0, 0)), ((64, 36), (128 * 8, 64 * 8 + 16), (0, 8)),
                                                    ((1, 1), (None, None), (0, 0)), ((4, 3), (None, None), (0, 0))])
def test_resolve_against_the_restatement(hip_ctx, extent, pitches, offsets):
    w, h = extent
    lit_np = gen.resolve_input(w, h, 5 * w + h) if w >= 3 else np.random.default_rng(1).integers(0, 0x7c00, (2 * h, 2 * w, 4), dtype=np.uint16)
    got = _resolve(hip_ctx, lit_np, pitches, offsets)
    if extent == gen.RESOLVE_EXTENT:
        fx = np.load(gen.FIXTURE)
        assert _resolve(hip_ctx, fx["resolve_in"], pitches, offsets).tobytes() == fx["resolve_out"].tobytes()
    if w >= 3:
        assert (got == 0x7e00).any() and (got == 0x7c00).any() and (got == 0x7bff).any()  # the non-finite cases are in
    for rows in ((0, 1), (h // 2, h), (h, h), (1, max(1, h - 1))):
        _resolve(hip_ctx, lit_np, pitches, offsets, rows)


def test_resolve_of_a_variable_rate_frame(hip_ctx):
    """the mode end to end on one case: lighting at 64 x 36 through the rate image, resolved to 32 x 18"""
    c = _case(hip_ctx, 1, _abi.SHADOW_MODE_CSM, _abi.GI_LPV)
    got = _resolve(hip_ctx, c.run(hip_ctx))
    assert got.tobytes() == ref.resolve(c.want()).tobytes()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(hip_ctx):
    """every item of the header's list, on the device: its code, nothing launched (tests/vrs_fuzz_child.py fuzzes the same on a context
    without a device)"""
    import torch
    c = _case(hip_ctx, 0, _abi.SHADOW_MODE_CSM, _abi.GI_LPV)
    p = Planes(c, 1, 1, rate_extra=0)
    INV, FMT, UNS = _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT, _abi.SAH_ERR_UNSUPPORTED
    rp = p.rate.plane

    def plane(**kw):
        q = _abi.Plane(rp.ptr, rp.width, rp.height, rp.row_pitch_bytes, rp.format)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def call(status, rate=rp, texel=c.texel, tol=ref.TOLERANCE, rows=(0, 0), edit=None):
        d, keep = p.describe(c, rows)
        if edit:
            keep.append(edit(d))
        with pytest.raises(lib.SahError) as e:
            hip_ctx.lighting_vrs(d, rate, texel, tol)
        assert e.value.status == status, (e.value, status)

    call(FMT, plane(format=_abi.FORMAT_R8_UNORM))
    call(INV, plane(ptr=None))
    for texel in ((2, 8), (8, 128), (12, 8), (8, 0), (8, 24)):
        call(INV, texel=texel)
    call(INV, plane(width=rp.width - 1))
    call(INV, plane(height=rp.height - 2))  # (the plane has one row more than needed)
    call(INV, plane(row_pitch_bytes=rp.width - 1))
    call(INV, texel=(4, 8))  # the image is too small for smaller texels
    for tol in (-1e-9, float("nan"), float("-inf")):
        call(INV, tol=tol)
    for rows in ((2, 8), (4, 10), (8, 4), (0, 46), (43, 45)):
        call(INV, rows=rows)

    def no_lit(d):
        d.lit = None

    def lit_format(d):
        q = _abi.Plane(p.lit.plane.ptr, c.w, c.h, p.lit.pitch, _abi.FORMAT_R32_SFLOAT)
        d.lit = C.pointer(q)
        return q

    def lights(d):
        ll = _abi.LightList(c.dev["depth"].data_ptr(), 1)
        d.lights = C.pointer(ll)
        return ll

    def gi_kind(kind):
        def edit(d):
            d.gi.contents.kind = kind
        return edit
    call(INV, edit=no_lit)          # what sah_lighting refuses, with its codes
    call(FMT, edit=lit_format)
    call(INV, edit=gi_kind(7))
    call(UNS, edit=lights)
    call(UNS, edit=gi_kind(_abi.GI_CACHE))
    call(UNS, edit=gi_kind(_abi.GI_RTGI))
    v = _abi.LightingVrsDesc(None, C.pointer(rp), (C.c_uint32 * 2)(8, 8), 0.0)
    assert hip_ctx.lib.sah_lighting_vrs(hip_ctx.handle, C.byref(v)) == INV and hip_ctx.lib.sah_lighting_vrs(hip_ctx.handle, None) == INV
    d, keep = p.describe(c)
    v = _abi.LightingVrsDesc(C.pointer(d), None, (C.c_uint32 * 2)(8, 8), 0.0)
    assert hip_ctx.lib.sah_lighting_vrs(hip_ctx.handle, C.byref(v)) == INV and hip_ctx.lib.sah_lighting_vrs(None, C.byref(v)) == INV

    lit2 = Image(RGBA16F, 2 * c.w, 2 * c.h, None, None)

    def resolve(status, lit, out, rows=(0, 0)):
        with pytest.raises(lib.SahError) as e:
            hip_ctx.vrsaa_resolve(lit, out, rows)
        assert e.value.status == status, (e.value, status)

    def edited(src, **kw):
        q = _abi.Plane(src.ptr, src.width, src.height, src.row_pitch_bytes, src.format)
        for k, val in kw.items():
            setattr(q, k, val)
        return q
    resolve(FMT, edited(lit2.plane, format=_abi.FORMAT_R16G16_SFLOAT), p.lit.plane)
    resolve(FMT, lit2.plane, edited(p.lit.plane, format=_abi.FORMAT_R8G8B8A8_UNORM))
    resolve(INV, edited(lit2.plane, width=2 * c.w - 1), p.lit.plane)      # an odd source extent
    resolve(INV, edited(lit2.plane, height=2 * c.h - 2), p.lit.plane)     # another ratio
    resolve(INV, p.lit.plane, p.lit.plane)
    resolve(INV, lit2.plane, edited(p.lit.plane, row_pitch_bytes=c.w * 8 - 8))
    resolve(INV, lit2.plane, edited(p.lit.plane, ptr=p.lit.plane.ptr + 4))
    resolve(INV, lit2.plane, p.lit.plane, (0, c.h + 1))
    resolve(INV, lit2.plane, p.lit.plane, (9, 3))
    assert hip_ctx.lib.sah_vrsaa_resolve(hip_ctx.handle, None, C.byref(p.lit.plane), 0, 0) == INV
    torch.cuda.synchronize()
    assert p.lit.unchanged() and lit2.unchanged() and p.inputs_unchanged()
