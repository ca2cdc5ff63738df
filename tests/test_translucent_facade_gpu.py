"""GPU: the layers above sah_translucent_render.  frame.rasterised_frame(translucent=...) with frame.Translucency, and TranslucencyPhase of the C++
host façade (tests/cpp/host_translucent.cpp, built by build(); compiled here when that program is missing), give the bytes of the direct calls;
with translucent=None — the default — and without the phase the frame is byte-identical to the frame as it was."""
import ctypes as C
import faulthandler
import os
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, mesh, scene, synth
from tests import translucent_ref as ref
from tests import util
from tests.host_programs import host_program

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 54
TORCH = {"color": "uint8", "normals": "int16", "data": "uint8", "emission": "uint8", "depth": "float32"}


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(300, exit=True)  # an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


def _new_gbuffer():
    import torch
    return {k: torch.full((H, W) + ((c,) if c else ()), 9, dtype=getattr(torch, TORCH[k]), device="cuda") for k, (c, _) in ref.GBUFFER_SHAPES.items()}


def _sorted_scene():
    """scene_panes with its translucent primitives shuffled, then ordered by the helper: the order the scene was written in"""
    arrays = ref.scene_panes().arrays()
    opaque, translucent = mesh.split_translucent(arrays)
    view = scene.SceneView.default(W, H)
    shuffled = dict(translucent, primitives=np.ascontiguousarray(translucent["primitives"][[3, 6, 0, 5, 2, 1, 4]]))
    ordered = mesh.sort_back_to_front(shuffled, view.gpu_data.view[:])
    assert ordered["primitives"].tobytes() == translucent["primitives"].tobytes(), "scene_panes lists its glass back to front"
    return opaque, ordered


def test_rasterised_frame_with_and_without_translucent(hip_ctx):
    import torch
    opaque, translucent = _sorted_scene()
    fr = ref.Frame(ref.HipBackend(hip_ctx), ref.scene_panes(), W, H)
    want, blended = fr.compose()
    ref.assert_preconditions(fr, want, blended, min_depth=3)
    f = fr.f
    dev = f.device_arrays()
    geo_o, geo_t = mesh.geometry(mesh.to_device(opaque), []), mesh.geometry(mesh.to_device(translucent), [])

    # the default: the frame as it was (the G-buffer of the opaque half; no Lighting, no blend)
    plain = _new_gbuffer()
    assert frame.rasterised_frame(hip_ctx, geo_o, f.view.gpu_data, plain) is None
    torch.cuda.synchronize()
    for k in ref.GBUFFER_KEYS:
        assert util.from_torch(plain[k], ref.GBUFFER_SHAPES[k][1]).tobytes() == np.ascontiguousarray(f.arrays[k]).tobytes(), k

    lit = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")

    def lighting(gbuffer):
        arrays = dict(dev)
        arrays.update(gbuffer)
        return f.describe(arrays, lit)
    gb = _new_gbuffer()
    t = {"pass": frame.Translucency(hip_ctx), "geometry": geo_t, "lighting": lighting}
    assert frame.rasterised_frame(hip_ctx, geo_o, f.view.gpu_data, gb, translucent=t) is None
    torch.cuda.synchronize()
    for k in ref.GBUFFER_KEYS:
        assert util.from_torch(gb[k], ref.GBUFFER_SHAPES[k][1]).tobytes() == util.from_torch(plain[k], ref.GBUFFER_SHAPES[k][1]).tobytes(), k
    got = util.from_torch(lit, np.uint16)
    assert got.tobytes() == want.tobytes() and got.tobytes() != fr.lit0.tobytes()
    assert t["pass"].deepest_pixel() == blended.max()
    # a band through the helper
    lit.copy_(util.to_torch(np.array(fr.lit0)))
    d, keep = lighting(gb)
    t["pass"](d, geo_t, rows=(10, 30))
    torch.cuda.synchronize()
    assert (d.row_begin, d.row_end) == (0, 0)
    assert util.from_torch(lit, np.uint16).tobytes() == np.concatenate([fr.lit0[:10], want[10:30], fr.lit0[30:]]).tobytes()


def test_translucency_phase_through_cpp_facade(tmp_path, hip_ctx):
    import torch
    steps = 1
    opaque, translucent = mesh.split_translucent(ref.scene_panes(textured=False).arrays())  # (the façade program uploads no textures)
    ao, luts = synth.ao_plane(W, H, 3), synth.sky_luts(7)
    vols = [v.view(np.uint16) for v in synth.lpv_volumes(4, 5)]
    pattern = np.random.default_rng(8).integers(0, 0x7bff, (H, W, 4), dtype=np.uint16)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as fh:
        fh.write(np.array([W, H, steps, len(opaque["positions"]), len(opaque["indices"]), len(opaque["materials"]), len(opaque["primitives"]),
                           len(translucent["primitives"])], np.uint32).tobytes())
        for a in (opaque["positions"], opaque["vertex_data"], opaque["indices"], opaque["materials"], opaque["primitives"], translucent["primitives"], ao,
                  luts["transmittance"], luts["sky_view"], pattern, *vols):
            fh.write(np.ascontiguousarray(a).tobytes())
    subprocess.check_call([host_program("host_translucent", tmp_path), str(inp), str(outp)], timeout=120)
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
    gb = {k: np.frombuffer(take(W * H * (c or 1) * np.dtype(dt).itemsize), dtype=dt).reshape((H, W) + ((c,) if c else ())).copy() for k, (c, dt) in ref.GBUFFER_SHAPES.items()}
    lit_plain, lit_glass, lit_alone = (np.frombuffer(take(W * H * 8), dtype=np.uint16).reshape(H, W, 4) for _ in range(3))
    assert off == len(blob)
    assert lit_alone.tobytes() == pattern.tobytes(), "the phase without a Lighting pass wrote to the lit image"

    # the direct calls on the blocks the C++ façade built
    geo_o, geo_t = mesh.geometry(mesh.to_device(opaque), []), mesh.geometry(mesh.to_device(translucent), [])
    dev_gb = _new_gbuffer()
    frame.rasterised_frame(hip_ctx, geo_o, view_c, dev_gb)
    torch.cuda.synchronize()
    for k in ref.GBUFFER_KEYS:
        assert util.from_torch(dev_gb[k], ref.GBUFFER_SHAPES[k][1]).tobytes() == gb[k].tobytes(), k
    f = util.LightingFrame(W, H, gbuffer=gb, seed=0, sun_mode=_abi.SHADOW_MODE_OFF, gi=_abi.GI_LPV)
    f.arrays["ao"] = ao
    f.arrays["sky_t"], f.arrays["sky_v"] = luts["transmittance"], luts["sky_view"]
    f.arrays["lpv_r"], f.arrays["lpv_g"], f.arrays["lpv_b"] = lpv_out
    f.view.gpu_data, f.sun.constants, f.lpv.matrices = view_c, sun_c, casc
    dev = f.device_arrays()
    full = f.run_hip(hip_ctx, dev)
    assert lit_plain.tobytes() == full.tobytes(), "without the phase the façade's frame is not the frame of the direct call"
    lit = util.to_torch(full.copy())
    d, keep = f.describe(dev, lit)
    hip_ctx.translucent_render(d, geo_t)
    torch.cuda.synchronize()
    direct = util.from_torch(lit, np.uint16)
    assert lit_glass.tobytes() == direct.tobytes()
    changed = (direct != full).any(-1)
    assert changed.mean() >= 0.2, f"only {changed.mean():.3f} of the pixels change"
