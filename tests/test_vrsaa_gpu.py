"""GPU: sah_vrsaa_measure_aliasing and sah_vrsaa_shading_rate_image (include/sah_vrsaa.h) against the numpy restatement
(tests/vrsaa_ref.py) and its committed fixture, bit for bit.  The contrast kernel's tile is 64 x 16 pixels."""
import faulthandler

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib, scene
from tests import util
from tests import vrsaa_ref as ref
from tests.support import context_state, differs, Image, side_stream_context

pytestmark = pytest.mark.gpu
FIXTURE = "tests/golden/vrsaa_97x61.npz"


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)  # each test under a limit of its own: an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def fixture():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), FIXTURE))


def _inputs(w, h, seed, specials=True):
    g = np.random.default_rng(seed)
    color = g.integers(0, 256, (h, w, 4), dtype=np.uint8)
    depth = g.random((h, w), dtype=np.float32)
    if specials and w * h >= 16:
        bits = depth.view(np.uint32)
        for b in (0x7f800000, 0xff800000, 0x7fc00000, 0x80000000, 0x00000123):
            bits[g.integers(0, h), g.integers(0, w)] = b
        bits[0, 0], bits[h - 1, w - 1] = 0x7f800000, 0xff800000
    return color, depth


def _measure(ctx, color, depth, pitches=(None, None, None), offsets=(0, 0, 0), rows=(0, 0), out=None):
    import torch
    h, w = depth.shape
    c = Image(_abi.FORMAT_R8G8B8A8_SRGB, w, h, pitches[0], color, offsets[0])
    d = Image(_abi.FORMAT_D32_SFLOAT, w, h, pitches[1], depth, offsets[1])
    o = out or Image(_abi.FORMAT_R16G16_SFLOAT, w, h, pitches[2], None, offsets[2])
    ctx.vrsaa_measure_aliasing(c.plane, d.plane, o.plane, rows)
    torch.cuda.synchronize()
    assert c.unchanged() and d.unchanged()
    return o


def _rates(ctx, contrast_bits, sri_extent, rates=ref.RATES, num=None, c_pitch=None, s_pitch=None):
    import torch
    ch, cw = contrast_bits.shape[:2]
    c = Image(_abi.FORMAT_R16G16_SFLOAT, cw, ch, c_pitch, contrast_bits)
    s = Image(_abi.FORMAT_R8_UINT, sri_extent[0], sri_extent[1], s_pitch)
    p = scene.shading_rate_params((cw, ch), sri_extent, rates)
    if num is not None:
        p.num_shading_rates = num
    ctx.vrsaa_shading_rate_image(c.plane, s.plane, p)
    torch.cuda.synchronize()
    assert c.unchanged() and s.padding_intact()
    return s.texels(np.uint8)


# ---- contrast ---------------------------------------------------------------------------------------------------------------------------
def test_contrast_fixture_bit_for_bit_and_repeatable(hip_ctx, fixture):
    got = _measure(hip_ctx, fixture["color"], fixture["depth"]).texels(np.uint16).reshape(61, 97, 2)
    assert np.array_equal(got, fixture["contrast"]), differs(got, fixture["contrast"])
    again = _measure(hip_ctx, fixture["color"], fixture["depth"]).texels(np.uint16).reshape(61, 97, 2)
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("extent", [(1, 1), (1, 9), (9, 1), (8, 8), (203, 131), (129, 33)])  # (129, 33): two tiles and one more pixel in both axes
def test_contrast_small_extents(hip_ctx, extent):
    w, h = extent
    color, depth = _inputs(w, h, 7 + w)
    got = _measure(hip_ctx, color, depth).texels(np.uint16).reshape(h, w, 2)
    want = ref.contrast(color, depth)
    assert np.array_equal(got, want), differs(got, want)


@pytest.mark.parametrize("pitches,offsets", [((97 * 4 + 12, 97 * 4 + 20, 97 * 4 + 4), (4, 8, 12)),  # no plane 16-byte aligned
                                             ((400, 416, 400), (0, 0, 0)),                              # padded, 16-byte aligned: the 16-byte stores
                                             ((512, 388, 392), (0, 4, 16))])
def test_contrast_pitches_sentinels_and_inputs(hip_ctx, fixture, pitches, offsets):
    out = _measure(hip_ctx, fixture["color"], fixture["depth"], pitches, offsets)  # (asserts the inputs unchanged)
    got = out.texels(np.uint16).reshape(61, 97, 2)
    assert np.array_equal(got, fixture["contrast"]), differs(got, fixture["contrast"])
    assert out.padding_intact()


def test_contrast_row_bands(hip_ctx, fixture):
    whole = _measure(hip_ctx, fixture["color"], fixture["depth"], (None, None, 416))
    out = Image(_abi.FORMAT_R16G16_SFLOAT, 97, 61, 416)
    for rows in ((20, 21), (0, 20), (21, 61)):
        before = out.bytes().copy()
        _measure(hip_ctx, fixture["color"], fixture["depth"], rows=rows, out=out)
        after = out.bytes()
        body = (after != before)[:61 * 416].reshape(61, 416)
        assert not body[:rows[0]].any() and not body[rows[1]:].any() and not body[:, 97 * 4:].any() and not (after != before)[61 * 416:].any()
    assert out.bytes().tobytes() == whole.bytes().tobytes()
    assert np.array_equal(out.texels(np.uint16).reshape(61, 97, 2), fixture["contrast"])
    # (k, k) with k > 0 is an empty band
    _measure(hip_ctx, fixture["color"], fixture["depth"], rows=(5, 5), out=out)
    assert out.bytes().tobytes() == whole.bytes().tobytes()


def test_contrast_all_nan_depth_is_the_luma_term(hip_ctx):
    w, h = 70, 19
    color, _ = _inputs(w, h, 3)
    depth = np.full((h, w), np.nan, np.float32)
    got = _measure(hip_ctx, color, depth).texels(np.uint16).reshape(h, w, 2)
    with np.errstate(all="ignore"):
        luma_term = (ref.gradients(ref.luma(color)) * np.float32(0.5)).astype(np.float16).view(np.uint16)
    assert np.array_equal(got, luma_term), differs(got, luma_term)
    assert np.array_equal(got, ref.contrast(color, depth))


def test_refusals_on_the_device(hip_ctx, fixture):
    """(the CPU test runs the whole list on a context without a device; here: a refusal launches nothing — the target keeps its bytes)"""
    c = Image(_abi.FORMAT_R8G8B8A8_SRGB, 97, 61, None, fixture["color"])
    d = Image(_abi.FORMAT_D32_SFLOAT, 97, 61, None, fixture["depth"])
    o = Image(_abi.FORMAT_R16G16_SFLOAT, 97, 61)
    s = Image(_abi.FORMAT_R8_UINT, 13, 8)
    for bad, status in (((c.plane, d.plane, _abi.Plane(o.plane.ptr, 97, 61, 97 * 4, _abi.FORMAT_R32_SFLOAT), (0, 0)), _abi.SAH_ERR_UNSUPPORTED_FORMAT),
                        ((c.plane, d.plane, o.plane, (0, 62)), _abi.SAH_ERR_INVALID_ARGUMENT),
                        ((c.plane, d.plane, o.plane, (9, 3)), _abi.SAH_ERR_INVALID_ARGUMENT),
                        ((c.plane, _abi.Plane(d.plane.ptr, 96, 61, 97 * 4, _abi.FORMAT_D32_SFLOAT), o.plane, (0, 0)), _abi.SAH_ERR_INVALID_ARGUMENT)):
        with pytest.raises(lib.SahError) as e:
            hip_ctx.vrsaa_measure_aliasing(*bad)
        assert e.value.status == status
    p = scene.shading_rate_params((97, 61), (13, 8), ref.RATES)
    p.num_shading_rates = 9
    with pytest.raises(lib.SahError) as e:
        hip_ctx.vrsaa_shading_rate_image(o.plane, s.plane, p)
    assert e.value.status == _abi.SAH_ERR_INVALID_ARGUMENT
    with pytest.raises(lib.SahError) as e:
        hip_ctx.vrsaa_shading_rate_image(o.plane, s.plane, scene.shading_rate_params((97, 61), (13, 9), ref.RATES))
    assert e.value.status == _abi.SAH_ERR_INVALID_ARGUMENT
    import torch
    torch.cuda.synchronize()
    assert o.unchanged() and s.unchanged()


# ---- shading-rate image -----------------------------------------------------------------------------------------------------------------
def _random_contrast(w, h, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    amp = ((xx * 7 // w) + (yy * 5 // h)) / 10.0  # flat to steep across the image: blocks of every size meet maxima under the search's saturation
    v = ((g.random((h, w, 2)) ** 3 * 1.2 - 0.2) * amp[..., None]).astype(np.float16)
    return v.view(np.uint16)


def test_shading_rate_fixture(hip_ctx, fixture):
    got = _rates(hip_ctx, fixture["contrast"], (13, 8))
    assert np.array_equal(got, fixture["shading_rate_image"]), differs(got, fixture["shading_rate_image"])


@pytest.mark.parametrize("cw,ch,sw,sh,d", [(119, 50, 8, 4, 15),   # blocks reach past the image on both axes
                                           (20, 20, 8, 8, 2),     # 2.5 rounds to even
                                           (5, 5, 7, 7, 1),       # zeros outside
                                           (256, 64, 16, 4, 16),  # the 16 x 16 block of a whole wave
                                           (300, 40, 3, 2, 100)])  # more texels per block than lanes
def test_shading_rate_block_sizes_and_out_of_range_reads(hip_ctx, cw, ch, sw, sh, d):
    assert ref.block_size(cw, sw) == d
    contrast = _random_contrast(cw, ch, cw)
    contrast[ch - 1, cw - 1] = np.array([2.0, 0.25], np.float16).view(np.uint16)  # the last texel counts where a block reaches it
    got = _rates(hip_ctx, contrast, (sw, sh))
    want = ref.shading_rate_image(contrast, (sw, sh), ref.RATES)
    assert np.array_equal(got, want), differs(got, want)
    assert len(np.unique(want)) >= 2


def test_shading_rate_special_contrast_values(hip_ctx):
    cw, ch, sw, sh = 64, 32, 16, 8  # d = 4
    contrast = _random_contrast(cw, ch, 11).view(np.float16) * np.float16(0.2)
    specials = np.array([np.inf, -np.inf, np.nan, -0.75, 65504.0, -65504.0, -0.0, 6e-8], np.float16)
    for k, v in enumerate(specials):
        contrast[4 * (k % 8) + 1, 4 * k + 2, k % 2] = v
    contrast[20:24, 8:12] = np.nan  # a block of nothing but NaN: m stays +0
    bits = np.ascontiguousarray(contrast).view(np.uint16)
    got = _rates(hip_ctx, bits, (sw, sh))
    want = ref.shading_rate_image(bits, (sw, sh), ref.RATES)
    assert np.array_equal(got, want), differs(got, want)
    assert want[5, 2] == 10


@pytest.mark.parametrize("num", [0, 1, 8])
def test_shading_rate_counts(hip_ctx, num):
    rates = [(2, 2), (1, 1), (1, 2), (2, 1), (2, 4), (4, 2), (4, 4), (1, 4)]
    contrast = _random_contrast(48, 24, 5)
    got = _rates(hip_ctx, contrast, (12, 6), rates, num)
    want = ref.shading_rate_image(contrast, (12, 6), rates, num_rates=num)
    assert np.array_equal(got, want), differs(got, want)
    if num < 2:
        assert (got == ref.rate_code(2, 2)).all()  # rates[0] whether the search runs over nothing or over itself


def test_shading_rate_first_of_equal_costs_wins(hip_ctx):
    flat = np.zeros((16, 16, 2), np.uint16)
    for rates in ([(2, 4), (4, 2)], [(4, 2), (2, 4)], [(2, 2), (4, 4), (4, 4), (1, 1)], [(1, 2), (2, 1), (1, 2)]):
        got = _rates(hip_ctx, flat, (4, 4), rates)
        assert np.array_equal(got, ref.shading_rate_image(flat, (4, 4), rates))
    assert (_rates(hip_ctx, flat, (4, 4), [(2, 4), (4, 2)]) == ref.rate_code(2, 4)).all()
    assert (_rates(hip_ctx, flat, (4, 4), [(4, 2), (2, 4)]) == ref.rate_code(4, 2)).all()
    steep = np.full((16, 16, 2), np.float16(1.0).view(np.uint16), np.uint16)  # saturated: optimal = (1, 1), and (1, 2), (2, 1) cost 1 each
    assert (_rates(hip_ctx, steep, (4, 4), [(1, 2), (2, 1)]) == ref.rate_code(1, 2)).all()
    assert (_rates(hip_ctx, steep, (4, 4), [(2, 1), (1, 2)]) == ref.rate_code(2, 1)).all()
    assert ref.rate_code(1, 2) != ref.rate_code(2, 1) and ref.rate_code(2, 4) != ref.rate_code(4, 2)


def test_shading_rate_pitches(hip_ctx, fixture):
    got = _rates(hip_ctx, fixture["contrast"], (13, 8), c_pitch=97 * 4 + 12, s_pitch=29)  # (_rates asserts sentinels and inputs)
    assert np.array_equal(got, fixture["shading_rate_image"])


# ---- both ---------------------------------------------------------------------------------------------------------------------------------
def _chain_images(fixture, color=None, depth=None):
    c = Image(_abi.FORMAT_R8G8B8A8_SRGB, 97, 61, None, fixture["color"] if color is None else color)
    d = Image(_abi.FORMAT_D32_SFLOAT, 97, 61, None, fixture["depth"] if depth is None else depth)
    return c, d, Image(_abi.FORMAT_R16G16_SFLOAT, 97, 61), Image(_abi.FORMAT_R8_UINT, 13, 8)


def test_chain_on_a_side_stream_without_host_sync_and_under_capture(fixture):
    import torch
    params = scene.shading_rate_params((97, 61), (13, 8), ref.RATES)
    with side_stream_context() as (ctx, s):
        c, d, o, r = _chain_images(fixture)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.vrsaa_measure_aliasing(c.plane, d.plane, o.plane)
            ctx.vrsaa_shading_rate_image(o.plane, r.plane, params)  # no host synchronisation in between
        s.synchronize()
        assert np.array_equal(o.texels(np.uint16).reshape(61, 97, 2), fixture["contrast"])
        assert np.array_equal(r.texels(np.uint8), fixture["shading_rate_image"])
        # one captured graph, a linear chain; replayed over other input contents
        color2, depth2 = _inputs(97, 61, 99)
        c2, d2, o2, r2 = _chain_images(fixture, color2, depth2)
        direct_o = ref.contrast(color2, depth2)
        direct_r = ref.shading_rate_image(direct_o, (13, 8), ref.RATES)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ctx.vrsaa_measure_aliasing(c.plane, d.plane, o.plane)
            ctx.vrsaa_shading_rate_image(o.plane, r.plane, params)
        c.t.copy_(c2.t)
        d.t.copy_(d2.t)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.vrsaa_measure_aliasing(c2.plane, d2.plane, o2.plane)
            ctx.vrsaa_shading_rate_image(o2.plane, r2.plane, params)
        s.synchronize()
        assert o.bytes().tobytes() == o2.bytes().tobytes() and r.bytes().tobytes() == r2.bytes().tobytes()
        assert np.array_equal(o.texels(np.uint16).reshape(61, 97, 2), direct_o) and np.array_equal(r.texels(np.uint8), direct_r)
        assert not np.array_equal(direct_o, fixture["contrast"])


def test_no_side_effects_on_the_context(hip_ctx, fixture):
    import torch
    f = util.LightingFrame(64, 36, seed=5, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, flavour="atrium")
    f.run_hip(hip_ctx)

    def state():
        return context_state(hip_ctx)
    before = state()
    c, d, o, r = _chain_images(fixture)
    hip_ctx.vrsaa_measure_aliasing(c.plane, d.plane, o.plane)
    hip_ctx.vrsaa_shading_rate_image(o.plane, r.plane, scene.shading_rate_params((97, 61), (13, 8), ref.RATES))
    torch.cuda.synchronize()
    assert state() == before
    assert np.array_equal(r.texels(np.uint8), fixture["shading_rate_image"])
