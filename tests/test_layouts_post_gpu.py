"""The post chain on pitched, offset images (tests/layouts.py): copy scene, the fused copy + bloom mip 0 launch, the bloom pyramid whole and
cut at mip 1, and both tonemap kernels — against the oracle on tight arrays by the bar of tests/test_post_gpu.py, against the same library on
tight images bit for bit, and with every padding byte checked.  Every image of a call has a padding of its own, so that a kernel which
addresses one image by another's pitch, or by width * 8, cannot pass."""
import ctypes as C
import functools

import numpy as np
import pytest

from androidrenderer_amd import _abi, images, synth
from tests import layouts, util
from tests.layouts import NAN_FILL, RGBA16F, SRGBA8

pytestmark = pytest.mark.gpu

SIZES = [(301, 171), (9, 5)]
OUT16, OUT8 = 0x7E01, 0x5A  # payload an output holds before the call: a NaN half / a code no test image is made of

# RGBA16F planes: base and pitch must be multiples of 8 (csrc/ctx.hpp: rgba16f_ok); the RGBA8 output: multiples of 4 (api_post.cpp: tonemap_args)
MIP_KEYS = [f"mip{i}" for i in range(6)]
LAYOUTS = {
    "A": dict({"lit": dict(row_pad=8, offset=8), "aa": dict(row_pad=8), "out": dict(row_pad=4)},
              **{k: dict(row_pad=8, offset=8 * (i % 2)) for i, k in enumerate(MIP_KEYS)}),
    "B": dict({"lit": dict(row_pad=24, offset=16), "aa": dict(row_pad=40, offset=8), "out": dict(row_pad=4, offset=4)},
              **{k: dict(row_pad=8 * (2 * i + 7), offset=8 * i) for i, k in enumerate(MIP_KEYS)}),  # 56, 72, 88, 104, 120, 136: none a multiple of 16
}
TIGHT = {}


def _mips_np(w, h, n=6):
    return [np.zeros((mh, mw, 4), np.uint16) for (mw, mh) in images.bloom_mip_sizes(w, h, n)]


def _p16(a):
    return images.plane(a, RGBA16F)


@functools.lru_cache(maxsize=None)
def _reference(w, h, nonfinite=False):
    """the oracle's post chain on tight arrays, once per extent: lit -> antialiased (same extent and 2x) -> six bloom mips -> tonemapped"""
    o = util.oracle()
    lit = synth.hdr_scene(w, h, seed=31)
    if nonfinite:  # as test_copy_scene_and_bloom_mip0_in_one_pass
        rng = np.random.default_rng(5)
        ys, xs = rng.integers(0, h, 60), rng.integers(0, w, 60)
        lit[ys[:20], xs[:20], :3] *= np.float16(-1.0)
        lit[ys[20:40], xs[20:40], 0] = np.float16(np.inf)
        lit[ys[40:], xs[40:], 1] = np.float16(np.nan)
    lit = lit.view(np.uint16)
    aa, aa2 = np.zeros((h, w, 4), np.uint16), np.zeros((2 * h, 2 * w, 4), np.uint16)
    assert o.orc_copy_scene(C.byref(_p16(lit)), C.byref(_p16(aa))) == 0
    assert o.orc_copy_scene(C.byref(_p16(lit)), C.byref(_p16(aa2))) == 0
    mips = _mips_np(w, h)
    assert o.orc_bloom(C.byref(_p16(aa)), C.byref(images.mipchain(mips))) == 0
    out = np.zeros((h, w, 4), np.uint8)
    assert o.orc_tonemap(C.byref(_p16(aa)), C.byref(images.mipchain(mips)), C.byref(images.plane(out, SRGBA8)), 0, 0) == 0
    return {"lit": lit, "aa": aa, "aa2": aa2, "mips": mips, "out": out}


def _in16(a, spec):
    """an RGBA16F input on the device; its padding reads as NaN halves"""
    return layouts.pitched(util.to_torch(a), RGBA16F, 2, spec, fill=NAN_FILL)


def _out16(shape, spec):
    import torch
    return layouts.pitched(torch.full(shape, OUT16, dtype=torch.int16, device="cuda"), RGBA16F, 2, spec, fill=NAN_FILL)


def _out8(shape, spec):
    import torch
    return layouts.pitched(torch.full(shape, OUT8, dtype=torch.uint8, device="cuda"), SRGBA8, 2, spec)


def _chain(ps):
    mc = _abi.MipChain()
    mc.num_mips = len(ps)
    for i, p in enumerate(ps):
        mc.mips[i] = p.plane()
    return mc


def _sync():
    import torch
    torch.cuda.synchronize()


# ---- copy scene -----------------------------------------------------------------------------------------------------------------------

def _hip_copy_scene(ctx, ref, scale, spec):
    lit = _in16(ref["lit"], spec.get("lit"))
    h, w = ref["lit"].shape[:2]
    out = _out16((scale * h, scale * w, 4), spec.get("aa"))
    ctx.copy_scene(lit.plane(), out.plane())
    _sync()
    layouts.assert_padding_intact(lit, out, what="copy_scene")
    layouts.assert_inputs_unchanged(lit, what="copy_scene")
    return out.read(np.uint16)


@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_copy_scene_on_pitched_planes(hip_ctx, size, scale, layout):
    ref = _reference(*size)
    want = ref["aa"] if scale == 1 else ref["aa2"]
    tight = _hip_copy_scene(hip_ctx, ref, scale, TIGHT)
    got = _hip_copy_scene(hip_ctx, ref, scale, LAYOUTS[layout])
    d = util.f16_ulp_diff(got, want)
    print(util.report_ulp(f"copy x{scale} {layout}", d))
    assert d.max() <= 1  # test_copy_scene's bar
    assert np.array_equal(got, tight)


# ---- copy scene + bloom mip 0 in one launch -------------------------------------------------------------------------------------------

def _hip_copy_bloom(ctx, ref, spec, parts=None):
    """-> (antialiased, mip 0, rows of each that were asked for)"""
    lit = _in16(ref["lit"], spec.get("lit"))
    aa = _out16(ref["aa"].shape, spec.get("aa"))
    mip = _out16(ref["mips"][0].shape, spec.get("mip0"))
    aa_rows, mip_rows = np.zeros(ref["aa"].shape[0], bool), np.zeros(ref["mips"][0].shape[0], bool)
    for (a0, a1), (m0, m1) in (parts or [((0, aa_rows.size), (0, mip_rows.size))]):
        ctx.copy_scene_bloom_mip0(lit.plane(), aa.plane(), _chain([mip]), (a0, a1), (m0, m1))
        aa_rows[a0:a1] = True
        mip_rows[m0:m1] = True
    _sync()
    layouts.assert_padding_intact(lit, aa, mip, what="copy_scene_bloom_mip0")
    layouts.assert_inputs_unchanged(lit, what="copy_scene_bloom_mip0")
    return aa.read(np.uint16), mip.read(np.uint16), aa_rows, mip_rows


@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("size", SIZES)
def test_copy_scene_bloom_mip0_on_pitched_planes(hip_ctx, size, layout):
    ref = _reference(*size, nonfinite=True)
    t_aa, t_mip, _, _ = _hip_copy_bloom(hip_ctx, ref, TIGHT)
    aa, mip, _, _ = _hip_copy_bloom(hip_ctx, ref, LAYOUTS[layout])
    assert np.array_equal(aa, ref["aa"]) and np.array_equal(mip, ref["mips"][0])
    assert np.array_equal(aa, t_aa) and np.array_equal(mip, t_mip)


@pytest.mark.parametrize("layout", ["A", "B"])
def test_copy_scene_bloom_mip0_row_ranges_on_pitched_planes(hip_ctx, layout):
    """the partitions of test_copy_scene_and_bloom_mip0_in_one_pass_row_ranges at 301 x 171 (mip 0: 150 x 85): a full partition, and single
    ranges whose other rows must keep what they held"""
    ref = _reference(301, 171)
    for parts in ([((0, 24), (0, 11)), ((20, 25), (11, 12)), ((21, 121), (12, 60)), ((119, 171), (60, 85))], [((60, 110), (40, 45))], [((75, 100), (40, 45))],
                  [((0, 171), (80, 85))], [((5, 6), (0, 85))]):
        t_aa, t_mip, _, _ = _hip_copy_bloom(hip_ctx, ref, TIGHT, parts)
        aa, mip, aa_rows, mip_rows = _hip_copy_bloom(hip_ctx, ref, LAYOUTS[layout], parts)
        assert np.array_equal(aa[aa_rows], ref["aa"][aa_rows]), parts
        assert np.array_equal(mip[mip_rows], ref["mips"][0][mip_rows]), parts
        assert (aa[~aa_rows] == OUT16).all() and (mip[~mip_rows] == OUT16).all(), parts
        assert np.array_equal(aa, t_aa) and np.array_equal(mip, t_mip), parts


@pytest.mark.parametrize("size", SIZES)
def test_copy_scene_bloom_mip0_fit_cache_across_layouts(hip_ctx, size):
    """The fused launch keeps the host's last 'does it fit' answer per thread under a key that holds the lit pitch and no other
    (csrc/post.hip: launch_copy_bloom_mip0).  The same extents on one thread: tight, padded lit only, padded aa and mip 0 only, tight again —
    every call gives the oracle's image, whatever the call before it left in the cache."""
    ref = _reference(*size)
    b = LAYOUTS["B"]
    for step, spec in (("tight", TIGHT), ("padded lit", {"lit": b["lit"]}), ("padded aa and mip 0", {"aa": b["aa"], "mip0": b["mip0"]}), ("tight again", TIGHT)):
        aa, mip, _, _ = _hip_copy_bloom(hip_ctx, ref, spec)
        assert np.array_equal(aa, ref["aa"]), step
        assert np.array_equal(mip, ref["mips"][0]), step


# ---- the bloom pyramid ------------------------------------------------------------------------------------------------------------------

def _hip_bloom(ctx, ref, spec, cut=None):
    """sah_bloom, or (cut = m) sah_bloom_mip_rows over a partition of every mip up to m + sah_bloom_from_mip(m), as
    test_bloom_split_at_any_mip_equals_bloom cuts it"""
    scene = _in16(ref["aa"], spec.get("aa"))
    mips = [_out16(m.shape, spec.get(k)) for k, m in zip(MIP_KEYS, ref["mips"])]
    chain = _chain(mips)
    if cut is None:
        ctx.bloom(scene.plane(), chain)
    else:
        for m in range(cut + 1):
            rows = ref["mips"][m].shape[0]
            cuts = sorted({0, rows // 3, rows // 3 + 1, (2 * rows) // 3, rows})
            for r0, r1 in zip(cuts, cuts[1:]):
                ctx.bloom_mip_rows(scene.plane(), chain, m, r0, r1)
        ctx.bloom_from_mip(scene.plane(), chain, cut)
    _sync()
    layouts.assert_padding_intact(scene, mips, what="bloom")
    layouts.assert_inputs_unchanged(scene, what="bloom")
    return [m.read(np.uint16) for m in mips]


@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("cut", [None, 1])
@pytest.mark.parametrize("size", SIZES)
def test_bloom_on_pitched_planes(hip_ctx, size, cut, layout):
    ref = _reference(*size)
    tight = _hip_bloom(hip_ctx, ref, TIGHT, cut)
    got = _hip_bloom(hip_ctx, ref, LAYOUTS[layout], cut)
    for i, (a, t, want) in enumerate(zip(got, tight, ref["mips"])):
        assert np.array_equal(a, want), f"mip {i} {a.shape}: {util.report_ulp('bloom', util.f16_ulp_diff(a, want))}"
        assert np.array_equal(a, t), f"mip {i}"


# ---- tonemap ------------------------------------------------------------------------------------------------------------------------------

def _bands(h):
    """four row bands, cut like those of test_tonemap_row_shards (117 rows: 27 / 54 / 85)"""
    cuts = sorted({0, (27 * h) // 117, (54 * h) // 117, (85 * h) // 117, h})
    return list(zip(cuts, cuts[1:]))


def _hip_tonemap(ctx, scene_np, mips_np, out_shape, spec, flags, rows=None):
    scene = _in16(scene_np, spec.get("aa"))
    mips = [_in16(m, spec.get(k)) for k, m in zip(MIP_KEYS, mips_np)]
    out = _out8(out_shape, spec.get("out"))
    for r0, r1 in (rows or [(0, 0)]):
        ctx.tonemap(scene.plane(), _chain(mips), out.plane(), r0, r1, flags=flags)
    _sync()
    layouts.assert_padding_intact(scene, mips, out, what="tonemap")
    layouts.assert_inputs_unchanged(scene, mips, what="tonemap")
    return out.read(np.uint8)


def _assert_tonemap(ctx, scene_np, mips_np, want, spec, rows, share=True):
    strict_t = _hip_tonemap(ctx, scene_np, mips_np, want.shape, TIGHT, 0, rows)
    strict = _hip_tonemap(ctx, scene_np, mips_np, want.shape, spec, 0, rows)
    assert np.array_equal(strict, want), f"{int((strict != want).sum())} of {want.size} codes differ from the oracle"
    assert np.array_equal(strict, strict_t)
    tol_t = _hip_tonemap(ctx, scene_np, mips_np, want.shape, TIGHT, _abi.TONEMAP_TOLERANCE_1CODE, rows)
    tol = _hip_tonemap(ctx, scene_np, mips_np, want.shape, spec, _abi.TONEMAP_TOLERANCE_1CODE, rows)
    d = np.abs(strict.astype(np.int32) - tol.astype(np.int32))
    print(f"tolerance mode: max |code difference| {int(d.max())}, share at 1: {float((d == 1).mean()):.5f}")
    assert d.max() <= 1  # test_tonemap_tolerance_mode_within_one_code's bar
    if share:
        assert (d == 1).mean() < 0.01
    assert np.array_equal(tol, tol_t)


@pytest.mark.parametrize("layout", ["A", "B"])  # (the output: rows 4 bytes apart in alignment, so every other row is not 8-byte aligned; B also shifts the base by 4)
@pytest.mark.parametrize("banded", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_tonemap_on_pitched_planes(hip_ctx, size, banded, layout):
    ref = _reference(*size)
    _assert_tonemap(hip_ctx, ref["aa"], ref["mips"], ref["out"], LAYOUTS[layout], _bands(size[1]) if banded else None)


@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("case", ["one_mip", "output_smaller"])
def test_tonemap_unusual_chains_on_pitched_planes(hip_ctx, case, layout):
    """test_tonemap_unusual_chains' two cases in which the kernel leaves its usual staging: absent mips alias the (pitched) scene; a smaller
    output falls back to the per-pixel filter"""
    o = util.oracle()
    w, h = 192, 108
    ow, oh = (120, 70) if case == "output_smaller" else (w, h)
    n = 1 if case == "one_mip" else 6
    scene = synth.hdr_scene(w, h, seed=29).view(np.uint16)
    mips = _mips_np(w, h)
    assert o.orc_bloom(C.byref(_p16(scene)), C.byref(images.mipchain(mips))) == 0
    mips = mips[:n]
    want = np.zeros((oh, ow, 4), np.uint8)
    assert o.orc_tonemap(C.byref(_p16(scene)), C.byref(images.mipchain(mips)), C.byref(images.plane(want, SRGBA8)), 0, 0) == 0
    # (test_tonemap_tolerance_mode_rows_and_unusual_chains asks for one code, not for the share, in these cases)
    _assert_tonemap(hip_ctx, scene, mips, want, LAYOUTS[layout], None, share=False)
