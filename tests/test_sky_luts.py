"""Sky LUT generators (transmittance, multiple scattering, sky view — sah_sky_update_luts).
CPU: physical sanity / known answers of the oracle.  GPU: HIP == oracle (bar: <= 1 ULP of the stored fp16, the tolerance of
BASELINE.json's north_star; the transcendentals are fp64 libm values on both sides, so equality is the expectation), and the
generated LUTs drive a Lighting pass with a sky."""
import ctypes as C

import numpy as np
import pytest

from androidrenderer_amd import _abi, images
from tests import util

LIGHT = (0.3, -0.8, 0.52)  # direction the sun light travels (normalisation is not required by the shader)


def _oracle_luts(light=LIGHT):
    o = util.oracle()
    t, m, s = np.zeros((64, 256, 4), np.uint16), np.zeros((32, 32, 4), np.uint16), np.zeros((200, 200, 4), np.uint16)
    planes = [images.plane(a, _abi.FORMAT_R16G16B16A16_SFLOAT) for a in (t, m, s)]
    assert o.orc_sky_update_luts(C.byref(planes[0]), C.byref(planes[1]), C.byref(planes[2]), (C.c_float * 3)(*light)) == 0
    return t, m, s


def _f(a):
    return a.view(np.float16).astype(np.float32)


def test_transmittance_lut_known_answers():
    t, _, _ = _oracle_luts()
    T = _f(t)
    assert (T[..., 3] == 1.0).all() and np.isfinite(T).all() and T[..., :3].min() >= 0.0 and T[..., :3].max() <= 1.0
    # row 63 (v = 63/64, near the top of the atmosphere), column 255 (sun almost at the zenith): nothing left to absorb
    assert np.allclose(T[63, 255, :3], 1.0, atol=2e-3)
    # looking straight down from any height hits the planet: exactly 0 (transmittance_lut.comp:17-20)
    assert (T[1:, 0, :3] == 0.0).all()
    # at a fixed sun angle transmittance grows with height, and blue is absorbed more than red (Rayleigh 6.6 < 12.3 < 29.4)
    col = T[:, 200, :3]
    assert (np.diff(col[:, 0]) >= -1e-3).all() and col[0, 0] > col[0, 1] > col[0, 2]


def test_multiscattering_and_sky_view_are_finite_positive_and_blue_at_the_zenith():
    _, m, s = _oracle_luts()
    M, S = _f(m), _f(s)
    assert np.isfinite(M).all() and np.isfinite(S).all() and M[..., :3].min() >= 0.0 and S[..., :3].min() >= 0.0
    assert 0.01 < M[..., :3].max() < 1.0 and 0.01 < S[..., :3].max() < 2.0
    zenith = S[199, 100, :3]
    assert zenith[2] > zenith[1] > zenith[0]  # Rayleigh sky
    assert S[100, 100, :3].sum() > zenith.sum()  # brighter towards the horizon (v = 0.5 is the horizon row)


def test_sky_view_follows_the_sun():
    _, _, day = _oracle_luts((0.0, -1.0, 0.0))      # sun overhead
    _, _, dusk = _oracle_luts((0.0, -0.05, 1.0))    # sun near the horizon
    assert _f(day)[..., :3].mean() > 1.2 * _f(dusk)[..., :3].mean()
    assert _f(day)[199, 100, :3].sum() > 2.0 * _f(dusk)[199, 100, :3].sum()  # the zenith is much darker at dusk


@pytest.mark.gpu
@pytest.mark.parametrize("light", [LIGHT, (0.0, -1.0, 0.0), (-0.7, -0.1, -0.7)])
def test_hip_sky_luts_match_oracle(hip_ctx, light):
    import torch
    want = _oracle_luts(light)
    dev = [torch.zeros(a.shape, dtype=torch.int16, device="cuda") for a in want]
    planes = [images.plane(a, _abi.FORMAT_R16G16B16A16_SFLOAT) for a in dev]
    hip_ctx.sky_update_luts(planes[0], planes[1], planes[2], light)
    torch.cuda.synchronize()
    for name, w, g in zip(("transmittance", "multiscattering", "sky_view"), want, dev):
        d = util.f16_ulp_diff(util.from_torch(g, np.uint16), w)
        print(util.report_ulp(name, d))
        assert d.max() <= 1, util.report_ulp(name, d)
        assert (d > 0).mean() < 1e-3, util.report_ulp(name, d)


@pytest.mark.gpu
def test_generated_luts_feed_the_sky_fill(hip_ctx):
    """End to end: LUTs generated on the device are the `sky` input of sah_lighting; the oracle gets the oracle's LUTs."""
    import torch
    f = util.LightingFrame(160, 90, seed=61, sun_mode=_abi.SHADOW_MODE_RT, gi=_abi.GI_NONE, flavour="atrium")
    sd = np.array(f.sun.constants.direction_and_tan_size[:3], dtype=np.float32)
    t, _, s = _oracle_luts(tuple(float(v) for v in sd))
    f.arrays["sky_t"], f.arrays["sky_v"] = t.view(np.float16), s.view(np.float16)
    want = f.run_oracle()
    dev = f.device_arrays()
    luts = [torch.zeros(shape, dtype=torch.int16, device="cuda") for shape in ((64, 256, 4), (32, 32, 4), (200, 200, 4))]
    planes = [images.plane(a, _abi.FORMAT_R16G16B16A16_SFLOAT) for a in luts]
    hip_ctx.sky_update_luts(planes[0], planes[1], planes[2], sd)
    dev["sky_t"], dev["sky_v"] = luts[0], luts[2]
    got = f.run_hip(hip_ctx, dev)
    d = util.f16_ulp_diff(got, want)
    assert d.max() <= 1, util.report_ulp("lighting with generated sky LUTs", d)
    sky = f.arrays["depth"] == 0
    assert sky.any() and (got[sky][:, :3] != 0).any()


# ---- pitched, offset targets (tests/layouts.py) -------------------------------------------------------------------------------------------
# RGBA16F: base and pitch multiples of 8 (csrc/ctx.hpp: rgba16f_ok); R32F: of 4 (csrc/api_probes.cpp: sah_ao_clear)
SKY_LAYOUTS = {"A": [dict(row_pad=8, offset=8), dict(row_pad=8), dict(row_pad=8, offset=16)],
               "B": [dict(row_pad=24), dict(row_pad=40, offset=8), dict(row_pad=56, offset=24)]}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["A", "B"])
def test_hip_sky_luts_into_pitched_planes(hip_ctx, layout):
    import torch
    from tests import layouts
    want = _oracle_luts(LIGHT)
    results = []
    for specs in ([None] * 3, SKY_LAYOUTS[layout]):
        dev = [layouts.pitched(torch.full(a.shape, 0x7e01, dtype=torch.int16, device="cuda"), _abi.FORMAT_R16G16B16A16_SFLOAT, 2, s, fill=layouts.NAN_FILL)
               for a, s in zip(want, specs)]
        hip_ctx.sky_update_luts(dev[0].plane(), dev[1].plane(), dev[2].plane(), LIGHT)
        torch.cuda.synchronize()
        layouts.assert_padding_intact(dev, what="sky_update_luts")
        results.append([p.read(np.uint16) for p in dev])
    for name, w, t, g in zip(("transmittance", "multiscattering", "sky_view"), want, *results):
        d = util.f16_ulp_diff(g, w)
        assert d.max() <= 1, util.report_ulp(name, d)            # test_hip_sky_luts_match_oracle's bar
        assert (d > 0).mean() < 1e-3, util.report_ulp(name, d)
        assert np.array_equal(g, t), name


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [dict(row_pad=4, offset=4), dict(row_pad=20, offset=12)])
def test_hip_ao_clear_into_a_pitched_plane(hip_ctx, spec):
    import torch
    from tests import layouts
    for w, h in ((161, 91), (9, 5)):
        ao = layouts.pitched(torch.full((h, w), 7.0, dtype=torch.float32, device="cuda"), _abi.FORMAT_R32_SFLOAT, 2, spec)
        hip_ctx.ao_clear(ao.plane())
        torch.cuda.synchronize()
        layouts.assert_padding_intact(ao, what="ao_clear")
        assert (ao.read(np.float32).view(np.uint32) == np.float32(1.0).view(np.uint32)).all()
