"""GPU: the C++ host façade's variable-rate option (LightingPhase::set_variable_rate_shading, VRSAA::resolve — tests/cpp/host_lighting_vrs.cpp,
built by build(); compiled here when that program is missing) and frame.VrsaaFrame.  Both produce the bytes of the direct calls; with the
option off — the default — the façade's frame is the frame it writes today, shading-rate image passed or not."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, images, scene, synth
from tests import lighting_vrs_ref as ref
from tests import util
from tests.host_programs import host_program

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGBA16F = _abi.FORMAT_R16G16B16A16_SFLOAT


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)  # an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


def _direct(ctx, fr, dev, rates, texel, tol):
    """(full, variable rate, resolve) by the direct calls"""
    import torch
    full = fr.run_hip(ctx, dev)
    lit = torch.zeros((fr.height, fr.width, 4), dtype=torch.int16, device="cuda")
    out = torch.zeros((fr.height // 2, fr.width // 2, 4), dtype=torch.int16, device="cuda")
    d, keep = fr.describe(dev, lit)
    sri = util.to_torch(rates)
    ctx.lighting_vrs(d, images.plane(sri, _abi.FORMAT_R8_UINT), texel, tol)
    ctx.vrsaa_resolve(images.plane(lit, RGBA16F), images.plane(out, RGBA16F))
    torch.cuda.synchronize()
    return full, util.from_torch(lit, np.uint16), util.from_torch(out, np.uint16)


def test_variable_rate_lighting_and_resolve_through_cpp_facade(tmp_path, hip_ctx):
    W, H, texel, steps, sun_mode = 76, 46, (8, 8), 1, _abi.SHADOW_MODE_RT  # the frame: twice an output of 38 x 23
    view = scene.SceneView.default(W, H)
    g = synth.atrium_gbuffer(W, H, view, seed=2)
    g["depth"] = ref.block_depth(W, H, 77)
    rates = ref.rate_image(W, H, texel, 1)
    ao, mask, luts = synth.ao_plane(W, H, 3), synth.shadow_mask(W, H, 4), synth.sky_luts(7)
    vols = [v.view(np.uint16) for v in synth.lpv_volumes(4, 5)]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([W, H, sun_mode, steps, texel[0], texel[1]], dtype=np.uint32).tobytes())
        f.write(np.array([ref.TOLERANCE], np.float32).tobytes())
        for a in (g["color"], g["normals"], g["data"], g["emission"], g["depth"], ao, mask, luts["transmittance"], luts["sky_view"], *vols, rates):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.check_call([host_program("host_lighting_vrs", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    off = 0

    def take(n):
        nonlocal off
        b = blob[off:off + n]
        off += n
        return b

    view_c = _abi.ViewData.from_buffer_copy(take(432))
    sun_c = _abi.SunLightConstants.from_buffer_copy(take(640))
    casc = (_abi.LpvCascadeMatrices * 4).from_buffer_copy(take(1024))
    lpv_out = [np.frombuffer(take(128 * 32 * 32 * 8), dtype=np.uint16).reshape(32, 32, 128, 4).copy() for _ in range(3)]
    lit_default, lit_vrs, lit_no_image = (np.frombuffer(take(W * H * 8), dtype=np.uint16).reshape(H, W, 4) for _ in range(3))
    resolved = np.frombuffer(take((W // 2) * (H // 2) * 8), dtype=np.uint16).reshape(H // 2, W // 2, 4)
    assert off == len(blob)

    # the direct calls on the blocks the C++ façade built
    fr = util.LightingFrame(W, H, gbuffer=g, seed=0, sun_mode=sun_mode, gi=_abi.GI_LPV)
    fr.arrays["ao"], fr.arrays["shadow_mask"] = ao, mask
    fr.arrays["sky_t"], fr.arrays["sky_v"] = luts["transmittance"], luts["sky_view"]
    fr.arrays["lpv_r"], fr.arrays["lpv_g"], fr.arrays["lpv_b"] = lpv_out
    fr.view.gpu_data, fr.sun.constants, fr.lpv.matrices = view_c, sun_c, casc
    full, vrs, res = _direct(hip_ctx, fr, fr.device_arrays(), rates, texel, ref.TOLERANCE)
    assert lit_default.tobytes() == full.tobytes(), "with the option off the façade's frame is not the full-rate frame"
    assert lit_no_image.tobytes() == full.tobytes(), "the option without an image is not the full-rate frame"
    assert lit_vrs.tobytes() == vrs.tobytes() and resolved.tobytes() == res.tobytes()
    sy, sx = ref.source_map(g["depth"], rates, texel, ref.TOLERANCE)
    assert vrs.tobytes() == full[sy, sx].tobytes() and vrs.tobytes() != full.tobytes()
    assert res.tobytes() == ref.resolve(vrs).tobytes()


def test_vrsaa_frame_helper(hip_ctx):
    import torch
    w, h, texel = 32, 18, (16, 16)
    depth, rates = ref.parity_inputs(1)  # 64 x 36
    fr = util.LightingFrame(2 * w, 2 * h, seed=9, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, sky=True)
    fr.arrays["depth"] = depth
    dev = fr.device_arrays()
    full, vrs, res = _direct(hip_ctx, fr, dev, rates, texel, ref.TOLERANCE)
    helper = frame.VrsaaFrame(hip_ctx, w, h, texel, ref.TOLERANCE)
    out = helper.render(fr, dev, util.to_torch(rates))
    torch.cuda.synchronize()
    assert out is helper.antialiased and tuple(out.shape) == (h, w, 4)
    assert util.from_torch(helper.lit, np.uint16).tobytes() == vrs.tobytes() and util.from_torch(out, np.uint16).tobytes() == res.tobytes()
    assert vrs.tobytes() != full.tobytes()
    with pytest.raises(ValueError):
        frame.VrsaaFrame(hip_ctx, w + 1, h, texel).render(fr, dev, util.to_torch(rates))
