"""Lighting's inputs beyond the G-buffer planes and the LPV volumes (those are tests/lighting_cases.py's `planes-*` and `lpv-*` cases) on pitched,
offset images: the CSM shadow map, the two sky LUTs, the three irradiance-cache atlases (the hot form gathers from an fp32 copy of the
irradiance atlas "with every pitch x 4", csrc/lighting_gi_ext.hpp), the RTGI ray planes and the noise of the extra rays.  Each: within
util.MAX_ULP of the oracle on tight arrays, bit-equal to the library on tight images, on the same kernel family as the tight run, nothing
written outside a payload, every input as uploaded."""
import numpy as np
import pytest

from androidrenderer_amd import _abi
from tests import layouts, lighting_cases as lc, util

pytestmark = pytest.mark.gpu

W, H = 160, 96
NAN = layouts.NAN_FILL  # fp16 / fp32 padding reads as NaN: a padding texel that reaches a pixel poisons it

# The Lighting pass checks no alignment of these inputs beyond what its hot forms ask for (csrc/api.cpp): A is the texel size — 2 bytes for the
# D16 shadow map, 8 for RGBA16F, 4 for the packed irradiance and RG16F depth atlases and the RGBA8 noise, 1 byte of row padding for the R8
# validity atlas; B: multiples of the texel size that are no multiples of 16, slice paddings that are no multiples of the row pitch.
CASES = {
    "csm_lpv_shadowmap": (dict(sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, seed=71), {
        "A": {"shadowmap": dict(row_pad=2, offset=2, slice_pad=2)},
        "B": {"shadowmap": dict(row_pad=6, offset=4, slice_pad=50)}}),
    "rt_sun_sky": (dict(sun_mode=_abi.SHADOW_MODE_RT, gi=_abi.GI_NONE, sky=True, seed=72), {
        "A": {"sky_t": dict(row_pad=8, offset=8, fill=NAN), "sky_v": dict(row_pad=8, fill=NAN)},
        "B": {"sky_t": dict(row_pad=24, fill=NAN), "sky_v": dict(row_pad=72, offset=40, fill=NAN)}}),
    "gi_cache": (dict(sun_mode=_abi.SHADOW_MODE_RT, gi=_abi.GI_CACHE, seed=73), {
        "A": {"probe_irr": dict(row_pad=4, offset=4, slice_pad=4), "probe_depth": dict(row_pad=4, slice_pad=4, fill=NAN), "probe_val": dict(row_pad=1, offset=4, slice_pad=1)},
        "B": {"probe_irr": dict(row_pad=20, slice_pad=100), "probe_depth": dict(row_pad=12, offset=4, slice_pad=52, fill=NAN), "probe_val": dict(row_pad=3, offset=8, slice_pad=7)}}),
    "gi_rtgi": (dict(sun_mode=_abi.SHADOW_MODE_RT, gi=_abi.GI_RTGI, num_extra_rays=3, seed=74), {
        "A": {"ray_buffer": dict(row_pad=8, offset=8, fill=NAN), "ray_irr": dict(row_pad=8, fill=NAN), "noise": dict(row_pad=4, offset=4)},
        "B": {"ray_buffer": dict(row_pad=24, fill=NAN), "ray_irr": dict(row_pad=56, offset=8, fill=NAN), "noise": dict(row_pad=12)}}),
}
_frames = {}


def _frame(name):
    """the case's frame and the oracle's image of it (tight arrays), once per session"""
    if name not in _frames:
        f = lc.MatrixFrame(W, H, flavour="atrium", **CASES[name][0])
        _frames[name] = (f, f.run_oracle())
    return _frames[name]


@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("name", list(CASES))
def test_lighting_inputs_on_pitched_images(hip_ctx, name, layout):
    f, want = _frame(name)
    spec = CASES[name][1][layout]
    assert set(spec) <= set(f.arrays), (set(spec), set(f.arrays))
    if name == "rt_sun_sky":
        assert (f.arrays["depth"] == 0).any()  # there is sky to fill
    try:
        f.pitch = {}
        tight = f.run_hip(hip_ctx)
        rep_tight = hip_ctx.lighting_dispatch()
        f.pitch = spec
        dev = f.device_arrays()
        assert all(isinstance(dev[k], lc.Pitched) and dev[k].row_pitch > dev[k].row_bytes for k in spec)
        got = f.run_hip(hip_ctx, dev)  # (asserts the padding itself)
        rep = hip_ctx.lighting_dispatch()
    finally:
        f.pitch = {}
    layouts.assert_inputs_unchanged(dev, what=name)
    print(f"{name} {layout}: tight {rep_tight}, padded {rep}")
    assert rep["family"] == rep_tight["family"], (rep, rep_tight)  # the padded layout is not quietly handed to another kernel family
    d = util.f16_ulp_diff(got, want)
    assert d.max() <= util.MAX_ULP, util.report_ulp(f"{name} {layout}", d)
    assert np.array_equal(got, tight), f"{name} {layout}: {int((got != tight).any(-1).sum())} pixels depend on the layout"
